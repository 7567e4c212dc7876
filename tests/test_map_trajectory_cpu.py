"""CPU: the restatement of the MAP trajectory (tests/map_trajectory_ref.py) against brute-force enumeration of all N^T paths, its
tie rule, the workspace sizes of the two entry-point families, and the cap on near-ties for every case tests/test_gpu_map_trajectory.py
runs (there on the device's forward arrays, here on the restatement's own)."""
import numpy as np
import pytest

import device_map_smoother_ref as S
import localization_ref as R
import map_trajectory_ref as V
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
def test_recursion_finds_the_best_of_all_paths(kind):
    X, W, lp_of = _small(kind)
    res = V.recursion(X, W, lp_of)
    path, score = V.brute_force(np.stack([V.log_weights(w) for w in W]), [lp_of(t) for t in range(4)])
    np.testing.assert_array_equal(res["path"], path)
    assert res["score"] == score and np.isfinite(float(score))
    assert res["delta"].dtype == LD and res["path"].shape == (5,)


def test_exact_ties_go_to_the_lowest_index():
    rs = np.random.RandomState(5)
    T, N = 4, 6
    X = rs.standard_normal((T, 3, N))
    X[:, :, 4] = X[:, :, 1]                                               # particle 4 duplicates particle 1 at every step
    W = rs.random_sample((T, N)) + 0.1
    W[:, 4] = W[:, 1]
    W[1, 2] = 0.0
    W /= W.sum(axis=1, keepdims=True)
    cov = 0.5 * np.eye(3)
    res = V.recursion(X, W, lambda t: V.lp_gauss(X[t + 1], X[t], cov, (0, 1, 2)))
    assert not np.any(res["psi"] == 4) and not np.any(res["path"] == 4)   # 1 and 4 tie exactly everywhere: 1 wins
    np.testing.assert_array_equal(res["delta"][:, 4], res["delta"][:, 1])
    assert res["delta"][1, 2] == -np.inf and res["psi"][1, 2] == 0        # w = 0: delta = -inf, psi = 0
    assert not np.any(res["psi"][2] == 2)                                 # ... and no successor comes from it
    assert not res["multi"].any()                                         # bit-identical columns count as one particle
    best, arg, near = V.step(np.full(N, -np.inf), np.zeros((N, 3)))
    assert np.all(best == -np.inf) and np.all(arg == 0)
    best, arg, near = V.step(np.zeros(N), np.zeros((N, 2)))
    assert np.all(arg == 0) and all(n.size == N for n in near)


def _chunks(N):
    bx = (N + 255) // 256
    want = max(1, (1024 + bx - 1) // bx)
    C = min(max(((N + want - 1) // want + 255) // 256 * 256, 256), 2048)
    return (N + C - 1) // C


@pytest.mark.parametrize("N,T", [(1, 1), (300, 7), (513, 2), (8192, 6), (65536, 100)])
def test_workspace_bytes(rbpf, N, T):
    """Xhat [rows + 1][N], the chunk partials (best fp64, arg int32) [nchunks][N], two rows of delta, x_map [n_nonlin][N_T] and the
    score; psi int32 [N_T][N_P] and the path's index [N_T]."""
    def want(nN, rows):
        nch = _chunks(N)
        return 8 * ((rows + 1) * N + nch * N + 2 * N + nN * T + 1) + 4 * (nch * N + T * N + T)
    assert rbpf.loc_map_workspace_bytes(N, T) == want(7, 7)
    assert rbpf.device_map_map_workspace_bytes(3, 1, N, T) == want(3, 1)
    assert rbpf.device_map_map_workspace_bytes(8, 8, N, T) == want(8, 8)
    assert rbpf.device_map_map_workspace_bytes(8, 6, N, T, quat_pos=1) == want(8, 6)
    for bad in (lambda: rbpf.loc_map_workspace_bytes(0, T), lambda: rbpf.loc_map_workspace_bytes(N, 0),
                lambda: rbpf.device_map_map_workspace_bytes(3, 4, N, T), lambda: rbpf.device_map_map_workspace_bytes(8, 6, N, T, quat_pos=3)):
        with pytest.raises(rbpf.RBPFError) as ei:
            bad()
        assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG


@pytest.mark.parametrize("kind,name", V.FULL_RUNS)
def test_cap_on_the_full_runs(kind, name):
    X, W, res = V.full_reference(kind, name)
    print(f"{kind} {name}: near-tied entries {res['frac']:.4%}, on the path {res['on_path']}, score {float(res['score']):.6f}")
    assert X.shape[0] == V.N_T and X.shape[2] == V.N_P
    assert V.cap_ok(res)
    assert len(np.unique(res["path"])) > 1                                # a path through the cloud, not one slot


@pytest.mark.parametrize("family", V.PROBE_FAMILIES)
@pytest.mark.parametrize("N,M", V.PROBE_SHAPES)
def test_probe_inputs(family, N, M):
    p = V.probe(family, N, M)
    assert p["best"].shape == (M,) and len(p["near"]) == M
    assert all(p["arg"][j] in p["near"][j] for j in range(M))
    if N >= 64:
        assert np.all(p["delta"][:10] == -np.inf) and np.all(np.isfinite(p["best"].astype(np.float64)))
        assert np.mean([n.size == 1 for n in p["near"]]) >= 0.99        # the probes pin arg at (nearly) every j
