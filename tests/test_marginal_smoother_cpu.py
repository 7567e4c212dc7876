"""CPU: the restatement of the marginal smoothing weights (tests/marginal_smoother_ref.py) against the marginals of the
backward-simulation path law enumerated over all N^T paths, its normalisation, its last row, what a zero weight does, and the
workspace sizes of the two entry-point families."""
import numpy as np
import pytest

import device_map_smoother_ref as S
import localization_ref as R
import map_trajectory_ref as V
import marginal_smoother_ref as G
import pose_transition_ref as P

LD = np.longdouble


def _small(kind):
    """(X [5 x n x 4], W [5 x 4], lp_of) of one case of a family at N = 4, T = 5, on the restatement's forward pass."""
    if kind == "mag":
        c = R.loc_case(4, 5, 13)
        X, W = V.forward_mag(c)
        dt, Q = V.pages(c, 5)
        return X, W, lambda t: V.lp_mag(X[t + 1], X[t], c["odometry"][t], dt[t], Q[:, :, t])
    c = S.case("D", 4, 5) if kind == "gauss" else P.case("E", 4, 5)
    X, W, _ = S.forward_arrays(c)
    mus, covs = S.transition_arrays(c, X)
    return X, W, lambda t: V.lp_case(c, X[t + 1], mus[t], covs[t])


@pytest.mark.parametrize("kind", ["mag", "gauss", "pose"])
def test_weights_are_the_marginals_of_the_path_law(kind):
    X, W, lp_of = _small(kind)
    res = G.recursion(X, W, lp_of)
    want = G.path_law_marginals(np.stack([V.log_weights(w) for w in W]), [lp_of(t) for t in range(4)])
    err = float(np.max(np.abs(res["w_smooth"] - want)))
    print(f"{kind}: restatement vs enumeration of 4^5 paths {err:.2e}; mass - 1 {float(np.max(np.abs(res['mass'] - 1))):.2e}")
    assert res["w_smooth"].dtype == LD and res["w_smooth"].shape == (5, 4)
    assert err <= 1e-15
    assert float(np.max(np.abs(np.sum(res["w_smooth"], axis=1) - 1))) <= 1e-15      # every row sums to 1
    assert float(np.max(np.abs(res["mass"] - 1))) <= 1e-15                           # ... before its normalisation too
    np.testing.assert_array_equal(res["w_smooth"][4], W[4].astype(LD))               # the last row is w_{T-1}
    np.testing.assert_array_equal(res["logws"][4], V.log_weights(W[4]))
    assert float(np.max(np.abs(res["w_smooth"][:4] - W[:4]))) > 1e-6                 # not the filter's weights repeated


def test_a_zero_weight_stays_zero_and_passes_nothing_back():
    rs = np.random.RandomState(5)
    T, N = 4, 6
    X = rs.standard_normal((T, 3, N))
    W = rs.random_sample((T, N)) + 0.1
    W[2, 1] = 0.0
    W[1, 4] = 0.0
    W /= W.sum(axis=1, keepdims=True)
    cov = 0.5 * np.eye(3)
    run = lambda Y: G.recursion(Y, W, lambda t: V.lp_gauss(Y[t + 1], Y[t], cov, (0, 1, 2)))   # noqa: E731
    res = run(X)
    assert res["w_smooth"][2, 1] == 0 and res["logws"][2, 1] == -np.inf
    assert res["w_smooth"][1, 4] == 0
    assert float(np.max(np.abs(np.sum(res["w_smooth"], axis=1) - 1))) <= 1e-15
    # wherever the zero-weight particle of step 2 lies, the steps before it see the same weights: it passes nothing back
    Y = X.copy()
    Y[2][:, 1] += 7.0
    moved = run(Y)
    np.testing.assert_array_equal(moved["w_smooth"], res["w_smooth"])
    np.testing.assert_array_equal(moved["D"][0], res["D"][0])
    # one step: -inf in logws_next gives c = -inf; every logws_next = -inf gives lws = -inf everywhere
    lp = V.lp_gauss(X[1], X[0], cov, (0, 1, 2))
    lwn = np.log(W[1], where=W[1] > 0, out=np.full(N, -np.inf))
    D, c, lws = G.step(np.log(W[0]), lp, lwn)
    assert c[4] == -np.inf and np.all(np.isfinite(np.delete(c, 4).astype(np.float64))) and np.all(np.isfinite(D.astype(np.float64)))
    D2, c2, lws2 = G.step(np.log(W[0]), lp, np.full(N, -np.inf))
    assert np.all(c2 == -np.inf) and np.all(lws2 == -np.inf)
    np.testing.assert_array_equal(D2, D)
    lw0 = np.log(W[0])
    lw0[2] = -np.inf
    D3, _, lws3 = G.step(lw0, lp, lwn)
    assert lws3[2] == -np.inf and np.all(D3 < D)                          # a predecessor with w = 0 contributes to no D


@pytest.mark.parametrize("N,T", [(1, 1), (300, 7), (513, 2), (8192, 6), (65536, 100)])
def test_workspace_bytes(rbpf, N, T):
    """Xhat [rows + 1][N]; the chunk partials (m, s) [nchunks][N] (M = N: both passes have the chunking of the backward pass); two
    rows of log w_{.|T} and c; w_smooth [N_T][N_P]; mean [n_nonlin], cov [n_nonlin x n_nonlin], ess and mass of every step.  All
    fp64."""
    def want(nN, rows):
        bx = (N + 255) // 256
        per = max(1, (1024 + bx - 1) // bx)
        C = min(max(((N + per - 1) // per + 255) // 256 * 256, 256), 2048)
        nch = (N + C - 1) // C
        return 8 * ((rows + 1) * N + 2 * nch * N + 3 * N + T * N + (nN + nN * nN + 2) * T)
    assert rbpf.loc_marginal_workspace_bytes(N, T) == want(7, 7)
    assert rbpf.device_map_marginal_workspace_bytes(3, 1, N, T) == want(3, 1)
    assert rbpf.device_map_marginal_workspace_bytes(8, 8, N, T) == want(8, 8)
    assert rbpf.device_map_marginal_workspace_bytes(8, 6, N, T, quat_pos=1) == want(8, 6)
    for bad in (lambda: rbpf.loc_marginal_workspace_bytes(0, T), lambda: rbpf.loc_marginal_workspace_bytes(N, 0),
                lambda: rbpf.device_map_marginal_workspace_bytes(3, 4, N, T),
                lambda: rbpf.device_map_marginal_workspace_bytes(8, 6, N, T, quat_pos=3)):
        with pytest.raises(rbpf.RBPFError) as ei:
            bad()
        assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG


@pytest.mark.parametrize("family", G.PROBE_FAMILIES)
@pytest.mark.parametrize("N,M", [s for s in G.PROBE_SHAPES if s[0] <= 513])
def test_probe_inputs(family, N, M):
    """What gives the GPU probes their meaning: -inf on both sides from 64 on, finite answers elsewhere, the chunk layout the
    shapes are chosen for."""
    p = G.probe(family, N, M)
    assert p["D"].shape == (M,) and p["lws"].shape == (N,)
    assert np.all(np.isfinite(p["D"].astype(np.float64)))
    dead_i, dead_j = p["logw"] == -np.inf, p["logws_next"] == -np.inf
    np.testing.assert_array_equal(p["lws"] == -np.inf, dead_i)
    np.testing.assert_array_equal(p["c"] == -np.inf, dead_j)
    if N >= 64:
        assert dead_i.sum() == 20
    if M >= 64:
        assert dead_j.sum() == 2
    assert G.chunks(300, 70) == (256, 2) and G.chunks(257, 513) == (256, 2) and G.chunks(2304, 2304) == (256, 9)
