"""CPU: the restatement of the two-slice statistics (tests/pair_stats_ref.py) against the two-slice marginals of the
backward-simulation path law enumerated over all N^T paths; the row and column sums of xi; the residuals it takes from the three
families' checkers; transition_noise_estimate on hand-made statistics; the new ABI symbols and the workspace sizes."""
import os
import re

import numpy as np
import pytest

import device_map_smoother_ref as S
import localization_ref as R
import map_trajectory_ref as V
import marginal_smoother_ref as G
import pair_stats_ref as PS
import pose_transition_ref as P

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T = 4, 4


def _small(kind):
    """(X [4 x n x 4], W [4 x 4], lp_of, r_of_t) of one case of a family at N = 4, T = 4, on the restatement's forward pass."""
    if kind == "mag":
        c = R.loc_case(N, T, 13)
        X, W = V.forward_mag(c)
        dt, Q = V.pages(c, T)
        return (X, W, lambda t: V.lp_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t]),
                lambda t: PS.r_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t]))
    c = S.case("D", N, T) if kind == "gauss" else P.case("E", N, T)
    X, W, _ = S.forward_arrays(c)
    mus, covs = S.transition_arrays(c, X)
    return X, W, lambda t: V.lp_case(c, X[t + 1], mus[t], covs[t]), lambda t: PS.r_of_case(c, X[t + 1], mus[t], covs[t])


@pytest.mark.parametrize("kind", ["mag", "gauss", "pose"])
def test_xi_is_the_two_slice_marginal_of_the_path_law(kind):
    X, W, lp_of, r_of_t = _small(kind)
    res = PS.recursion(X, W, lp_of, r_of_t)
    lw = np.stack([V.log_weights(w) for w in W])
    one, two = PS.path_law_pairs(lw, [lp_of(t) for t in range(T - 1)])
    assert float(np.max(np.abs(one - G.path_law_marginals(lw, [lp_of(t) for t in range(T - 1)])))) == 0.0
    worst = 0.0
    for t in range(T - 1):
        D, c, lws = G.step(lw[t], lp_of(t), res["logws"][t + 1])
        xi = PS.xi_matrix(lw[t], c, lp_of(t), PS.log_mass(lws))
        assert xi.dtype == LD and xi.shape == (N, N)
        worst = max(worst, float(np.max(np.abs(xi - two[t]))))
        assert float(np.max(np.abs(np.sum(xi, axis=1) - res["w_smooth"][t]))) <= 1e-15        # rows: w_{t|T}
        fin = c > -np.inf
        assert fin.all()
        assert float(np.max(np.abs(np.sum(xi, axis=0) - res["w_smooth"][t + 1])[fin])) <= 1e-15    # columns: w_{t+1|T}
        assert abs(float(np.sum(xi)) - 1.0) <= 1e-15
        # the moments are those of xi and the residuals, pair by pair
        r = np.stack([r_of_t(t)(j) for j in range(N)], axis=2)                               # [n x N(i) x N(j)]
        S_ = np.einsum("ij,aij,bij->ab", xi, r, r)
        assert float(np.max(np.abs(S_ - res["S"][t]))) <= 1e-15 * max(1.0, float(np.max(np.abs(S_))))
        assert float(np.max(np.abs(np.einsum("ij,aij->a", xi, r) - res["m"][t]))) <= 1e-15
        assert abs(float(res["pair_mass"][t]) - 1.0) <= 1e-15
    print(f"{kind}: xi of the restatement vs enumeration of {N}^{T} paths {worst:.2e}")
    assert worst <= 1e-15


def test_a_dead_successor_and_a_dead_predecessor_carry_no_pair():
    rs = np.random.RandomState(5)
    n, M = 6, 5
    X = rs.standard_normal((2, 3, n))
    cov = 0.5 * np.eye(3)
    lp = V.lp_gauss(X[1][:, :M], X[0], cov, (0, 1, 2))
    logw = np.log(rs.random_sample(n) + 0.1)
    lwn = np.log(rs.random_sample(M) + 0.1)
    logw[2] = -np.inf
    lwn[4] = -np.inf
    r_of = PS.r_gauss(X[1][:, :M], X[0], cov, (0, 1, 2))
    res = PS.step(logw, lp, lwn, r_of)
    xi = PS.xi_matrix(logw, res["c"], lp, PS.log_mass(res["lws"]))
    assert np.all(xi[2] == 0) and np.all(xi[:, 4] == 0) and abs(float(np.sum(xi)) - 1.0) <= 1e-15
    assert abs(float(res["pair_mass"]) - 1.0) <= 1e-15
    # every c = -inf: nothing at all, and no NaN from log(mass) = -inf
    dead = PS.step(logw, lp, np.full(M, -np.inf), r_of)
    assert np.all(dead["S"] == 0) and np.all(dead["m"] == 0) and dead["pair_mass"] == 0 and dead["mass"] == 0


def test_the_residuals_of_the_three_checkers_agree():
    """Without a block pose_transition_ref.residual_vector is the plain statement: the un-whitened device_map_smoother_ref.residual must
    give it back; the dense-mag residual is model E's (pose_transition_ref.dense_mag_as_pose)."""
    p = G.probe("D", 300, 70)
    r_of = PS.r_of_probe(p)
    for j in (0, 33, 69):
        want = P.residual_vector(p["xs_next"][:, j], p["mu"], p["rows"], p["angle_rows"], None, LD)
        assert float(np.max(np.abs(r_of(j) - want))) <= 1e-17 * 1e2
    q = G.probe("mag", 300, 70)
    r_of = PS.r_of_probe(q)
    for j in (0, 69):
        r = r_of(j)
        assert r.shape == (6, 300)
        np.testing.assert_allclose(r[0:3].astype(np.float64), q["xs_next"][0:3, j:j + 1] - q["X"][0:3] - q["odo"][0:3, None], rtol=0, atol=1e-14)
        assert float(np.max(np.abs(r[3:6]))) <= np.pi                      # phi = logq of a unit quaternion


def test_transition_noise_estimate(rbpf):
    rs = np.random.RandomState(3)
    n, Pg = 3, 5
    A = rs.standard_normal((n, n, Pg))
    S_ = np.einsum("abt,cbt->act", A, A)
    dt = rs.uniform(0.5, 2.0, Pg)
    m = 0.1 * rs.standard_normal((n, Pg))
    want = sum(S_[:, :, t] / dt[t] for t in range(Pg)) / Pg
    np.testing.assert_allclose(rbpf.transition_noise_estimate(S_, dt), want, rtol=1e-14)
    np.testing.assert_allclose(rbpf.transition_noise_estimate(S_, 0.5), np.mean(S_, axis=2) / 0.5, rtol=1e-14)
    np.testing.assert_allclose(rbpf.transition_noise_estimate(S_, np.append(dt, 9.0)), want, rtol=1e-14)     # dt of every step: the first P
    Qc, bias = rbpf.transition_noise_estimate(S_, dt, m)
    np.testing.assert_allclose(Qc, sum((S_[:, :, t] - np.outer(m[:, t], m[:, t])) / dt[t] for t in range(Pg)) / Pg, rtol=1e-14)
    np.testing.assert_allclose(bias, m.mean(axis=1), rtol=1e-14)
    # exact statistics of a known Q give it back: S_t = dt_t Q
    Q = np.array([[2.0, 0.3], [0.3, 1.0]])
    np.testing.assert_allclose(rbpf.transition_noise_estimate(np.stack([d * Q for d in dt], axis=2), dt), Q, rtol=1e-14)
    np.testing.assert_allclose(rbpf.transition_noise_estimate(0.25 * Q, 0.25), Q, rtol=1e-14)               # one page as a matrix
    for bad in (lambda: rbpf.transition_noise_estimate(S_, dt[:3]), lambda: rbpf.transition_noise_estimate(S_, -1.0),
                lambda: rbpf.transition_noise_estimate(S_, dt, m[:, :2]), lambda: rbpf.transition_noise_estimate(np.zeros((2, 3, 4)), 1.0)):
        with pytest.raises(ValueError):
            bad()


NEW_SYMBOLS = ["rbpf_loc_pair_stats_smooth", "rbpf_loc_pair_stats_workspace_bytes", "rbpf_loc_pair_stats_step",
               "rbpf_loc_generic_pair_stats_begin", "rbpf_loc_generic_pair_stats_particles_device", "rbpf_loc_generic_pair_stats_step_device",
               "rbpf_loc_generic_pair_stats_finish", "rbpf_loc_generic_pair_stats_workspace_bytes", "rbpf_loc_generic_pair_stats_step"]


def test_the_new_symbols_are_declared_exported_and_bound(rbpf):
    lib = rbpf.load_library()
    src = open(os.path.join(ROOT, "include", "rbpf.h")).read()
    import importlib
    ffi = importlib.import_module(rbpf.__name__ + "._ffi")
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in ffi.EXPORTS and getattr(lib, name).argtypes is not None, name
    for name in ("particleTransitionStatisticsLocalization", "loc_pair_stats_step", "device_map_pair_stats_step", "transition_noise_estimate",
                 "loc_pair_stats_workspace_bytes", "device_map_pair_stats_workspace_bytes"):
        assert callable(getattr(rbpf, name))
    assert hasattr(rbpf.LocalizationSession, "transition_statistics")
    assert re.search(r"two-slice\W+pairwise\W+marginals", src) is None       # no longer listed as out of scope


@pytest.mark.parametrize("N_P,N_T", [(1, 1), (300, 7), (513, 2), (4352, 3), (8192, 6), (65536, 100)])
def test_workspace_bytes(rbpf, N_P, N_T):
    """The marginal pass's workspace, one vector of K = n_res (n_res + 3) / 2 + 1 doubles per workgroup of the statistics pass
    (predecessor blocks of 256 x successor chunks of backward_chunk_size), and a page of n_res^2 + n_res + 1 doubles per pair of steps."""
    def extra(n_res):
        blocks, chunks = PS.groups(N_P, N_P)
        return 8 * ((n_res * (n_res + 3) // 2 + 1) * blocks * chunks + (N_T - 1) * (n_res * n_res + n_res + 1))
    assert PS.groups(300, 70) == (2, 1) and PS.groups(513, 257) == (3, 2) and PS.groups(2304, 2304) == (9, 9) and PS.groups(4352, 4352) == (17, 17)
    assert PS.groups(65536, 65536) == (256, 32)
    assert rbpf.loc_pair_stats_workspace_bytes(N_P, N_T) == rbpf.loc_marginal_workspace_bytes(N_P, N_T) + extra(6)
    for nN, n_sel, qpos, n_res in ((3, 1, -1, 1), (8, 8, -1, 8), (8, 6, 1, 5), (7, 7, 3, 6), (4, 4, 0, 3)):
        assert rbpf.device_map_pair_stats_workspace_bytes(nN, n_sel, N_P, N_T, quat_pos=qpos) == \
            rbpf.device_map_marginal_workspace_bytes(nN, n_sel, N_P, N_T, quat_pos=qpos) + extra(n_res)
    for bad in (lambda: rbpf.loc_pair_stats_workspace_bytes(0, N_T), lambda: rbpf.loc_pair_stats_workspace_bytes(N_P, 0),
                lambda: rbpf.device_map_pair_stats_workspace_bytes(3, 4, N_P, N_T),
                lambda: rbpf.device_map_pair_stats_workspace_bytes(8, 6, N_P, N_T, quat_pos=3)):
        with pytest.raises(rbpf.RBPFError) as ei:
            bad()
        assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
