"""GPU: backward simulation by rejection sampling (csrc/rbpf_loc_reject.hpp; LocalizationSession.backward_simulate(method="rejection"),
rbpf_loc_backward_simulate_reject, rbpf_loc_generic_backward_reject_*, the probes loc_backward_reject_step and
device_map_backward_reject_step) against the restatement tests/loc_reject_ref.py.

Every fixture meets the restatement's conditions (tests/test_loc_reject_cpu.py: every margin at least 100 x its error measure, the fp64
and the long-double decisions equal), so every index and every accepted_at is compared and none is left out; the full sessions assert
the same conditions on the forward arrays they read back from the device before they compare."""
import warnings

import numpy as np
import pytest

import loc_reject_ref as J
import transition_sweep_ref as TS

pytestmark = pytest.mark.gpu


def _live(rbpf):
    return int(rbpf.load_library().rbpf_device_bytes_live())


def _probe(rbpf, p, u_try=None):
    u_try = p["u_try"] if u_try is None else u_try
    if p["kind"] == "mag":
        index, acc, _ = rbpf.loc_backward_reject_step(p["X"], p["w"], p["xs_next"], p["odo"], p["dt"], p["Q"], u_try, p["u"])
    else:
        index, acc, _ = rbpf.device_map_backward_reject_step(p["mu"], p["w"], p["xs_next"], p["cov"], u_try, p["u"], rows=p["rows"],
                                                             angle_rows=p["angle_rows"], quat_rows=p["quat_rows"])
    return index, acc


def _old_probe(rbpf, p):
    if p["kind"] == "mag":
        return rbpf.loc_backward_step(p["X"], p["w"], p["xs_next"], p["odo"], p["dt"], p["Q"], p["u"])[0]
    return rbpf.device_map_backward_step(p["mu"], p["w"], p["xs_next"], p["cov"], p["u"], rows=p["rows"], angle_rows=p["angle_rows"],
                                         quat_rows=p["quat_rows"])[0]


def _against_reference(rbpf, p):
    want = J.reference(p)
    assert J.conditions(want)[0]
    index, acc = _probe(rbpf, p)
    M = p["xs_next"].shape[1]
    assert index.shape == (M,) and acc.shape == (M,) and index.dtype == np.int32
    np.testing.assert_array_equal(acc, want["accepted_at"])
    np.testing.assert_array_equal(index, want["index"])
    assert np.all(p["w"][index] > 0)                                       # no zero-weight particle is ever returned
    return want


# ------------------------------------------------------------------------------------------------
# 1. the probes, mixed regime
# ------------------------------------------------------------------------------------------------
def test_probe_mixed_dense_mag(rbpf):
    p = J.mag_fixture()
    want = _against_reference(rbpf, p)
    acc, fb = J.shares(want)
    assert acc >= 0.2 and fb >= 0.2 and want["n_fallback"] > 256


@pytest.mark.parametrize("name", TS.NAMES)
def test_probe_mixed_every_term(rbpf, name):
    want = _against_reference(rbpf, J.sweep_fixture(name))
    acc, fb = J.shares(want)
    assert acc >= 0.2 and fb >= 0.2


# ------------------------------------------------------------------------------------------------
# 2. max_tries = 0 is the existing method, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["mag", "g3a", "p4a"])
def test_probe_without_tries_is_the_existing_probe(rbpf, base):
    p = J.mag_fixture() if base == "mag" else J.sweep_fixture(base)
    index, acc = _probe(rbpf, p, u_try=np.zeros((0, p["xs_next"].shape[1], 2)))
    np.testing.assert_array_equal(index, _old_probe(rbpf, p))
    assert np.all(acc == -1)


class _Mag:
    def __init__(self, rbpf):
        self.rbpf, self.c = rbpf, J.session_case("mag")

    def session(self):
        rbpf, c = self.rbpf, self.c
        mp = rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])
        return rbpf.LocalizationSession(mp, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], c["N_P"], c["dt"], rng=rbpf.ReplayRNG(c["U"], c["Z"]),
                                        keep_history=True, trace=True)

    def mus(self):
        return None


class _Gauss:
    def __init__(self, rbpf):
        import test_gpu_device_map_smoother as G
        self.rbpf, self.h = rbpf, G._handles("D", J.SESSION["N_P"], J.SESSION["N_T"])

    def session(self):
        return self.h.session(self.rbpf)

    def mus(self):
        """What the `mean` handle returned at its last N_T-1 calls, mus[t]."""
        return self.h.mus[-(J.SESSION["N_T"] - 1):][::-1]


class _Landmark:
    def __init__(self, rbpf):
        import test_gpu_landmark_map as G
        self.rbpf, self.G, self.p = rbpf, G, J.session_case("landmark")
        self.tw = G.Twin(self.p)

    def session(self):
        rbpf, p = self.rbpf, self.p
        self.tw.reset()
        tr = rbpf.DeviceTransition(self.tw.drift, rows=(0, 1, 2))
        return rbpf.LocalizationSession(self.G._map(rbpf, self.tw, p, tr), p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["N_P"], p["dt"],
                                        rng=self.G._rng(rbpf, p), keep_history=True, trace=True)

    def mus(self):
        return None


def _runner(rbpf, kind):
    return {"mag": _Mag, "gauss": _Gauss, "landmark": _Landmark}[kind](rbpf)


@pytest.mark.parametrize("kind", J.SESSION_KINDS)
def test_session_without_tries_is_all_pairs(rbpf, kind):
    r = _runner(rbpf, kind)
    T, M = J.SESSION["N_T"], 700
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with r.session() as s:
            s.advance(T)
            s.finish()
            rng = rbpf.PhiloxRNG(J.SESSION["seed"])
            old = s.backward_simulate(M, rng=rng)
            new = s.backward_simulate(M, rng=rng, method="rejection", max_tries=0,
                                      want=("xs_traj", "index", "traj_smooth_mean", "n_fallback", "n_tries"))
    for k in ("index", "xs_traj", "traj_smooth_mean"):
        np.testing.assert_array_equal(new[k], old[k])
    np.testing.assert_array_equal(new["n_fallback"], [M] * (T - 1) + [0])
    assert not np.any(new["n_tries"]) and new["n_tries"].dtype == np.int64


# ------------------------------------------------------------------------------------------------
# 3. nothing falls back
# ------------------------------------------------------------------------------------------------
def test_nothing_falls_back(rbpf):
    p = J.nothing_falls_back_fixture()
    want = J.reference(p)
    assert want["n_fallback"] == 0 and J.conditions(want)[0]
    _probe(rbpf, p)                                                        # (the library and its code objects are loaded)
    before = _live(rbpf)
    index, acc = _probe(rbpf, p)
    assert _live(rbpf) == before
    assert np.all(acc >= 0)                                                # n_fallback == 0
    np.testing.assert_array_equal(acc, want["accepted_at"])
    np.testing.assert_array_equal(index, want["index"])


# ------------------------------------------------------------------------------------------------
# 4. everything falls back for one trajectory
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["mag", "g3", "p3"])
def test_one_trajectory_out_of_reach(rbpf, base):
    p = J.mag_fixture() if base == "mag" else J.sweep_fixture(base)
    j = 77
    q = J.far_successor(p, j)
    index, acc = _probe(rbpf, q)
    assert acc[j] == -1
    assert index[j] == _old_probe(rbpf, q)[j]                              # the existing probe's draw for the same u
    want = J.reference(p)
    keep = np.arange(index.size) != j
    np.testing.assert_array_equal(index[keep], want["index"][keep])        # all others are unaffected
    np.testing.assert_array_equal(acc[keep], want["accepted_at"][keep])


# ------------------------------------------------------------------------------------------------
# 5. full sessions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", J.SESSION_KINDS)
def test_full_session(rbpf, kind):
    r = _runner(rbpf, kind)
    T, N, R, seed = J.SESSION["N_T"], J.SESSION["N_P"], J.SESSION["R"], J.SESSION["seed"]
    want_all = ("xs_traj", "index", "traj_smooth_mean", "n_fallback", "n_tries")
    base = _live(rbpf)
    outs = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with r.session() as s:
            s.advance(T)
            fwd = s.finish(extras=True)
            xn_fwd = s.history()
            s.sync()
            before = _live(rbpf)
            for M in J.SESSION["n_traj"]:                                 # 130 over 300 and 700 over 300
                outs[M] = s.backward_simulate(M, rng=rbpf.PhiloxRNG(seed), method="rejection", max_tries=R, want=want_all)
                assert _live(rbpf) == before                              # the workspace went back to the pool
            mus = r.mus()
            again = s.backward_simulate(700, rng=rbpf.PhiloxRNG(seed), method="rejection", max_tries=R, want=("index", "n_fallback", "n_tries"))
    assert _live(rbpf) == base
    assert fwd["first_degenerate_step"] == -1
    for k in ("index", "n_fallback", "n_tries"):                          # two runs with one seed are identical
        np.testing.assert_array_equal(again[k], outs[700][k])
    X = np.ascontiguousarray(np.transpose(xn_fwd, (2, 0, 1)))            # [T x n x N], the device's own forward particles
    W = np.ascontiguousarray(fwd["trace_w"].T)
    assert X.shape[2] == N
    sim = J.simulate(X, W, J.session_lp(kind, X, mus), seed, R, 700)
    ok, worst = J.simulate_holds(sim)
    print(f"{kind}: smallest margin / error {worst:.3g}; n_fallback {sim['n_fallback'].tolist()}, n_tries {sim['n_tries'].tolist()}")
    assert ok                                                             # the conditions, on the device's own forward arrays
    out = outs[700]
    np.testing.assert_array_equal(out["index"].T, sim["index"])
    np.testing.assert_array_equal(out["n_fallback"], sim["n_fallback"])
    np.testing.assert_array_equal(out["n_tries"], sim["n_tries"])
    assert np.all(sim["n_fallback"][:T - 1] > 0) and np.all(sim["n_fallback"][:T - 1] < 700)
    np.testing.assert_array_equal(out["xs_traj"], np.stack([X[t][:, out["index"][:, t]] for t in range(T)], axis=2))
    np.testing.assert_allclose(out["traj_smooth_mean"], np.mean(out["xs_traj"], axis=1), rtol=1e-12, atol=1e-12)
    # the counters are keyed by the trajectory: 130 trajectories are the first 130 of 700, with their own counts
    small = outs[130]
    np.testing.assert_array_equal(small["index"], out["index"][:130])
    acc700 = [st["accepted_at"] for st in sim["steps"]]
    np.testing.assert_array_equal(small["n_fallback"][:T - 1], [int(np.sum(a[:130] < 0)) for a in acc700])
    tries = [int(np.sum(np.where(a[:130] >= 0, a[:130] + 1, R))) for a in acc700]
    np.testing.assert_array_equal(small["n_tries"][:T - 1], tries)
    assert small["n_fallback"][T - 1] == 0 and small["n_tries"][T - 1] == 0


# ------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals(rbpf):
    r = _runner(rbpf, "mag")
    T = J.SESSION["N_T"]
    with r.session() as s:
        s.advance(T)
        s.finish()
        with pytest.raises(ValueError, match="loc_backward_reject_step"):   # a replay array: the probes take uniforms
            s.backward_simulate(5, rng=np.full((T, 5), 0.5), method="rejection", max_tries=4)
        with pytest.raises(ValueError, match="max_tries"):
            s.backward_simulate(5, method="rejection", max_tries=-1)
        with pytest.raises(ValueError, match="unknown method"):
            s.backward_simulate(5, method="metropolis")
        with pytest.raises(ValueError, match="unknown outputs"):
            s.backward_simulate(5, want=("index", "n_fallback"))          # the counters belong to method="rejection"
        lib = rbpf.load_library()
        status = lib.rbpf_loc_backward_simulate_reject(s.ctx, 5, 1, -1, None, None, None, None, None)
        assert status == rbpf.RBPF_ERR_INVALID_ARG
        out = s.backward_simulate(5, method="rejection", max_tries=2)      # the session is still usable
        assert out["index"].shape == (5, T)
    g = _runner(rbpf, "gauss")
    with g.h.session(rbpf, transition=False) as s:
        s.advance(T)
        s.finish()
        with pytest.raises(rbpf.RBPFError) as e:
            s.backward_simulate(5, method="rejection", max_tries=4)
        assert e.value.status == rbpf.RBPF_ERR_UNSUPPORTED
    with g.session() as s:
        s.advance(T)
        s.finish()
        with pytest.raises(ValueError, match="max_tries"):
            s.backward_simulate(5, method="rejection", max_tries=-1)
        lib = rbpf.load_library()
        rows = np.array([0, 1, 3], dtype=np.int32)
        import ctypes as C
        status = lib.rbpf_loc_generic_backward_reject_begin(s.ctx, 5, 1, -1, 3, rows.ctypes.data_as(C.POINTER(C.c_int32)), 4, -1)
        assert status == rbpf.RBPF_ERR_INVALID_ARG
        assert lib.rbpf_loc_generic_backward_reject_stats(s.ctx, None, None) == rbpf.RBPF_ERR_STATE   # no pass has finished
    with r.session() as s:                                                # steps not done
        s.advance(2)
        with pytest.raises(rbpf.RBPFError) as e:
            s.backward_simulate(5, method="rejection", max_tries=4)
        assert e.value.status == rbpf.RBPF_ERR_STATE
