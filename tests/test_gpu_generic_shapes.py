"""GPU: the generic (host-callback) family at model shapes the built-in families never have -- n_nonlin from 1 to 8, n_w and
n_odo different from n_nonlin, nLin < n_y and nLin = 1, block-lower storage with host-supplied Jacobians, fp32 banks, the packed
information matrices of the information form and its carried factors -- against the numpy oracle (which takes any model
object) and against the extended-precision batch posterior of a no-noise model (tests/generic_model.py), and the refusals of
the shapes the library does not take.

Tolerances as in tests/test_gpu_filter.py / tests/test_gpu_smoother.py: resampling and ancestor indices bit-exact, everything
else 1e-9 relative; fp32 banks 2e-5."""
import numpy as np
import pytest

import generic_model as gm
import rbpf_oracle as O
import test_gpu_filter as tf
import test_gpu_smoother as ts

pytestmark = pytest.mark.gpu
RTOL = 1e-9
FP32_TOL = 2e-5

def case(shape, N_P, N_T, N_K=1, seed=3, additive=False):
    m = gm.GenericModel(*shape, seed=seed, additive=additive)
    return m, gm.problem(m, N_P, N_T, N_K=N_K, seed=seed)


def oracle_run(kind, m, p, use_dynResNorm=True):
    """The oracle's filter ("filter"), covariance-form ("cov") or information-form ("info") smoother; cached in the problem."""
    cache = p.setdefault("oracle", {})
    key = (kind, use_dynResNorm)
    if key not in cache:
        rng = O.ReplayRNG(p["U"], p["Z"], p["Ufin"])
        a = (m, p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], p["N_P"])
        if kind == "filter":
            cache[key] = O.particleFilter(*a, p["dt"], rng, trace=True)
        else:
            f = O.particleSmoother if kind == "cov" else O.particleSmootherInformationForm
            cache[key] = f(*a, p["N_K"], p["dt"], rng, trace=True, use_dynResNorm=use_dynResNorm)
    return cache[key]


def device_filter(rbpf, m, p, **kw):
    dyn, meas, _, state = gm.handles(m, p)
    out = rbpf.particleFilter(dyn, meas, p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], p["N_P"],
                              p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"]), extras=True, **kw)
    assert state["calls"] == (p["y"].shape[0] - 1) * p["N_P"]
    return out


def device_smoother(rbpf, m, p, info_form, use_dynResNorm=True, **kw):
    dyn, meas, drn, state = gm.handles(m, p, use_dynResNorm)
    f = rbpf.particleSmootherInformationForm if info_form else rbpf.particleSmoother
    out = f(dyn, meas, drn, p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], p["N_P"], p["N_K"],
            p["dt"], rng=rbpf.ReplayRNG(p["U"], p["Z"], p["Ufin"]), extras=True, **kw)
    T, N = p["y"].shape[0], p["N_P"]
    assert state["calls"] == (T - 1) * (N + (p["N_K"] - 1) * (N - 1))
    return out


def filter_parity(rbpf, m, p, **kw):
    tf.check_filter(oracle_run("filter", m, p), device_filter(rbpf, m, p, **kw))


def smoother_parity(rbpf, m, p, info_form, use_dynResNorm=True, **kw):
    ref = oracle_run("info" if info_form else "cov", m, p, use_dynResNorm)
    ts.check(ref, device_smoother(rbpf, m, p, info_form, use_dynResNorm, **kw), p["N_K"])


def fp32_filter_parity(rbpf, m, p, **kw):
    """storage precision: every stored element carries a 6e-8 relative rounding per rewrite (tests/test_gpu_filter.py)."""
    ref, out = oracle_run("filter", m, p), device_filter(rbpf, m, p, **kw)
    ex, tr = out[8], ref["trace"]
    np.testing.assert_array_equal(ex["ai"][1:], tr["ai"][1:])
    assert tf.rel(ex["w"], tr["w"]) <= FP32_TOL
    assert tf.rel(out[1], ref["traj_mean"]) <= FP32_TOL and tf.rel(out[2], ref["xl_max"]) <= FP32_TOL
    assert tf.rel(out[4], ref["P_max"]) <= FP32_TOL
    assert tf.rel(ex["xl"], tr["xl"]) <= FP32_TOL and tf.rel(ex["P"], tr["P"]) <= FP32_TOL
    assert tf.rel(ex["P"], tr["P"]) > 1e-12                                  # it really is a different storage precision


# ------------------------------------------------------------------------------------------------
# oracle parity, shape by shape
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scalar_case():
    return case((1, 1, 1, 1, 1), 8, 8, N_K=3)


@pytest.mark.parametrize("path", ["filter", "cov", "info"])
def test_one_nonlinear_state_one_output_one_coefficient(rbpf, scalar_case, path):
    """(n_nonlin, n_w, n_odo, n_y, nLin) = (1, 1, 1, 1, 1): every matrix of the step is 1 x 1."""
    m, p = scalar_case
    if path == "filter":
        filter_parity(rbpf, m, p)
    else:
        smoother_parity(rbpf, m, p, info_form=path == "info")


@pytest.fixture(scope="module")
def wide_h_case():
    return case((2, 2, 2, 3, 2), 8, 8, N_K=3)


@pytest.mark.parametrize("path", ["filter", "cov", "info"])
def test_fewer_coefficients_than_outputs(rbpf, wide_h_case, path):
    """(2, 2, 2, 3, 2): nLin < n_y, H wider than tall (H P H' of rank 2 < 3; S = H P H' + R stays SPD through R)."""
    m, p = wide_h_case
    if path == "filter":
        filter_parity(rbpf, m, p)
    else:
        smoother_parity(rbpf, m, p, info_form=path == "info")


@pytest.fixture(scope="module")
def eight_state_case():
    return case((8, 8, 8, 3, 64), 8, 8, N_K=3, additive=True)


def test_eight_nonlinear_states_filter(rbpf, eight_state_case):
    """(8, 8, 8, 3, 64): the fixed [8] register arrays of the kernels filled to the last entry."""
    filter_parity(rbpf, *eight_state_case)


@pytest.mark.parametrize("chol_refresh", [0, 2, 5, 1000])
def test_eight_nonlinear_states_information_form_with_an_empty_dynResNorm(rbpf, eight_state_case, chol_refresh):
    """The additive default of an empty dynResNorm (particleSmoother.m:175-177) at n_w = n_nonlin = 8; chol_refresh 0 (the
    from-scratch factorisation for a generic model) and carried factors refreshed every 2nd / 5th step or never (1000 >= N_T - 1),
    whose exactly carried information matrices are advanced by the gather kernel every step."""
    m, p = eight_state_case
    smoother_parity(rbpf, m, p, info_form=True, use_dynResNorm=False, chol_refresh=chol_refresh)


@pytest.fixture(scope="module")
def border_case():
    return case((5, 2, 4, 1, 129), 8, 8, N_K=3)


@pytest.mark.parametrize("lazy_depth", [0, 3])
def test_n_w_below_n_odo_below_n_nonlin_filter(rbpf, border_case, lazy_depth):
    """(5, 2, 4, 1, 129): n_w < n_odo < n_nonlin, n_y = 1, one core chunk and one border row; the lazy update's pending
    downdates use the Jacobians of past steps of a host-callback model."""
    filter_parity(rbpf, *border_case, lazy_depth=lazy_depth)


@pytest.mark.parametrize("info_form", [False, True])
def test_n_w_below_n_odo_below_n_nonlin_smoothers(rbpf, border_case, info_form):
    smoother_parity(rbpf, *border_case, info_form=info_form)


@pytest.fixture(scope="module")
def packed_case():
    return case((4, 3, 4, 3, 200), 6, 7, N_K=2)


@pytest.mark.parametrize("chol_refresh", [1, 5])
def test_information_form_with_packed_information_matrices(rbpf, packed_case, chol_refresh):
    """(4, 3, 4, 3, 200): nLin >= 176, the information matrices packed through the 64-column factorisation; from scratch every
    step and carried factors (the gather kernel on full squares beside the sweep)."""
    smoother_parity(rbpf, *packed_case, info_form=True, chol_refresh=chol_refresh)


@pytest.fixture(scope="module")
def four_tile_rows():
    return case((4, 3, 4, 3, 256), 10, 8)


@pytest.mark.parametrize("lazy_depth,inplace", [(0, 0), (3, 0), (4, 0), (3, 1)])
def test_block_lower_storage_without_border_rows(rbpf, four_tile_rows, lazy_depth, inplace):
    """(4, 3, 4, 3, 256): block-lower fp64 storage (four tile rows, no border row) with host-supplied Jacobians; the lazy
    update at depth 3 / 4 and one bank rewritten in place."""
    filter_parity(rbpf, *four_tile_rows, storage="fp64sym", lazy_depth=lazy_depth, inplace=inplace)


@pytest.fixture(scope="module")
def four_tile_rows_full_border():
    return case((3, 3, 3, 3, 383), 8, 7, N_K=2)


@pytest.mark.parametrize("lazy_depth,inplace", [(3, 0), (4, 0), (3, 1)])
def test_block_lower_storage_with_127_border_rows(rbpf, four_tile_rows_full_border, lazy_depth, inplace):
    filter_parity(rbpf, *four_tile_rows_full_border, storage="fp64sym", lazy_depth=lazy_depth, inplace=inplace)


def test_information_form_on_block_lower_storage_with_127_border_rows(rbpf, four_tile_rows_full_border):
    smoother_parity(rbpf, *four_tile_rows_full_border, info_form=True, storage="fp64sym")


@pytest.fixture(scope="module")
def eight_tile_rows():
    return case((6, 4, 6, 3, 639), 8, 6)


def test_eight_tile_rows_fp64_block_lower(rbpf, eight_tile_rows):
    filter_parity(rbpf, *eight_tile_rows, storage="fp64sym")


@pytest.mark.parametrize("storage", ["fp32sym", "fp32"])
def test_eight_tile_rows_fp32_banks(rbpf, eight_tile_rows, storage):
    """fp32 banks of a generic n_y = 3 filter: block-lower tiles and full squares."""
    fp32_filter_parity(rbpf, *eight_tile_rows, storage=storage)


@pytest.fixture(scope="module")
def two_tile_rows():
    return case((2, 1, 2, 1, 128), 10, 8, N_K=2)


def test_two_tile_rows_block_lower_filter(rbpf, two_tile_rows):
    """(2, 1, 2, 1, 128): the n_y = 1 block-lower layout (two tile rows, no border)."""
    filter_parity(rbpf, *two_tile_rows, storage="fp64sym")


def test_two_tile_rows_block_lower_information_form(rbpf, two_tile_rows):
    smoother_parity(rbpf, *two_tile_rows, info_form=True, storage="fp64sym")


@pytest.fixture(scope="module")
def sixteen_tile_rows():
    return case((3, 3, 3, 3, 1151), 6, 6)


def test_sixteen_tile_rows_fp64_block_lower(rbpf, sixteen_tile_rows):
    filter_parity(rbpf, *sixteen_tile_rows, storage="fp64sym")


def test_sixteen_tile_rows_fp32_block_lower(rbpf, sixteen_tile_rows):
    fp32_filter_parity(rbpf, *sixteen_tile_rows, storage="fp32sym")


def test_largest_carried_factor_size(rbpf):
    """(3, 3, 3, 3, 575): the largest nLin the carried factors take, chol_refresh = 5, information matrices advanced by the
    gather kernel."""
    m, p = case((3, 3, 3, 3, 575), 6, 7, N_K=2)
    smoother_parity(rbpf, m, p, info_form=True, chol_refresh=5)


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def _refused(rbpf, fn):
    with pytest.raises(rbpf.RBPFError) as ei:
        fn()
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED, ei.value
    return str(ei.value)


@pytest.mark.parametrize("shape", [(3, 3, 3, 2, 16), (9, 3, 9, 3, 16), (3, 9, 3, 3, 16)])
def test_shapes_outside_the_generic_family_are_refused(rbpf, shape):
    """n_y = 2, n_nonlin = 9, n_w = 9 (the device's fixed register arrays and small-matrix inverses)."""
    m, p = case(shape, 4, 3)
    _refused(rbpf, lambda: device_filter(rbpf, m, p))


def test_carried_factors_above_575_are_refused(rbpf):
    m, p = case((3, 3, 3, 3, 576), 4, 3, N_K=2)
    assert "575" in _refused(rbpf, lambda: device_smoother(rbpf, m, p, info_form=True, chol_refresh=5))


def test_info_rebuild_is_refused_for_a_generic_model(rbpf):
    """The rebuild from the state history needs measModel on the device."""
    m, p = case((3, 3, 3, 3, 40), 4, 3, N_K=2)
    _refused(rbpf, lambda: device_smoother(rbpf, m, p, info_form=True, chol_refresh=5, info_rebuild=1))


def test_fp32_tiles_at_four_tile_rows_are_refused(rbpf):
    m, p = case((4, 3, 4, 3, 256), 4, 3)
    _refused(rbpf, lambda: device_filter(rbpf, m, p, storage="fp32sym"))


def test_generic_smoother_on_sixteen_tile_rows_is_refused(rbpf):
    m, p = case((3, 3, 3, 3, 1100), 4, 3, N_K=2)
    _refused(rbpf, lambda: device_smoother(rbpf, m, p, info_form=True, storage="fp64sym"))


def test_fp32_smoother_of_a_generic_model_is_refused(rbpf):
    m, p = case((6, 4, 6, 3, 639), 4, 3, N_K=2)
    assert "filter" in _refused(rbpf, lambda: device_smoother(rbpf, m, p, info_form=True, storage="fp32sym"))


# ------------------------------------------------------------------------------------------------
# extended-precision known answer (no oracle)
# ------------------------------------------------------------------------------------------------
KAT_T = {256: 150, 639: 120, 1151: 100, 128: 150}


KAT_RUNS = [(shape, storage, lazy_depth) for shape in ((4, 3, 4, 3, 256), (6, 4, 6, 3, 639), (3, 3, 3, 3, 1151))
            for storage in ("fp64", "fp64sym") for lazy_depth in (0, 4)] + [((2, 1, 2, 1, 128), "fp64sym", 0),
                                                                          ((2, 1, 2, 1, 128), "fp64sym", 4)]


@pytest.mark.parametrize("shape,storage,lazy_depth", KAT_RUNS)
def test_device_kalman_recursion_equals_the_long_double_batch_posterior(rbpf, shape, storage, lazy_depth):
    """No process noise and one x0_lin column: every particle follows the same deterministic path, so after N_T sequential
    Kalman updates (particleFilter.m:184-198) each particle's xl and P are the batch posterior
        P_T = (P0^-1 + sum_t H_t' R^-1 H_t)^-1,   xl_T = P_T (P0^-1 x0 + sum_t H_t' R^-1 y_t),
    and the sum over t of its unnormalised log-weights (:139-150) is log N(y; Phi x0, Phi P0 Phi' + kron(I, R)).  The answer is
    computed in long double from the H_t of the path the device returns (generic_model.batch_posterior), not by the oracle.

    Tolerance (generic_model.kat_tolerance): 8 (M kappa(C) + N_T) u with M = n_y N_T and kappa(C) the 2-norm condition number of
    the batch innovation covariance -- the forward error of a backward-stable solve with C, which the recursion performs one
    block at a time, plus one rounding of P per step; P on the scale of P0, xl on the scale of the posterior mean and of its
    move from x0, the log-likelihood on |loglik| + M.  kappa ~ 1e3 at these problems: about 2e-10 to 4e-10, against the
    1e-7 / 1e-6 of test_device_kalman_recursion_equals_batch_gp_posterior."""
    N_T, N_P = KAT_T[shape[4]], 4
    m, p, ref = gm.kat_case(shape, N_P, N_T)
    out = device_filter(rbpf, m, p, storage=storage, lazy_depth=lazy_depth)
    xn_traj, ex = out[7], out[8]
    np.testing.assert_array_equal(xn_traj, np.repeat(gm.path_of(m, p)[:, None, :], N_P, axis=1))
    tol = gm.kat_tolerance(ref, N_T)
    assert tol < 1e-9
    xl, P, ll = ref["xl"].astype(np.float64), ref["P"].astype(np.float64), float(ref["loglik"])
    xscale = np.max(np.abs(xl)) + np.max(np.abs(xl - p["x0_lin"]))
    logw = np.asarray(ex["logw"])
    logw = logw if logw.shape[0] == N_P else logw.T
    for i in range(N_P):
        assert np.max(np.abs(ex["xl"][:, i] - xl)) <= tol * xscale, (i, np.max(np.abs(ex["xl"][:, i] - xl)) / xscale)
        assert np.max(np.abs(ex["P"][:, :, i] - P)) <= tol * ref["P0max"], (i, np.max(np.abs(ex["P"][:, :, i] - P)) / ref["P0max"])
        assert abs(float(np.sum(logw[i])) - ll) <= tol * (abs(ll) + ref["M"]), (i, float(np.sum(logw[i])), ll)
