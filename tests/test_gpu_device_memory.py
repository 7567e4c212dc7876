"""The library's own books of device memory balance: rbpf_device_bytes_live() -- the bytes all DevicePools of the process own --
is back at its earlier value, exactly, after every kind of session and one-shot call, refused creations included.  (Free
memory as the runtime reports it is no leak test on a shared device; the library's counter is.)  Small sizes: N_P <= 64, short T."""
import importlib

import numpy as np
import pytest

import cases
import localization_ref as R

pytestmark = pytest.mark.gpu


def _live(rbpf):
    return int(rbpf.load_library().rbpf_device_bytes_live())


def _mag(rbpf, N_P=32, N_T=8, m=130, N_K=1, seed=3):
    c = cases.mag_case(N_P, N_T, m, seed=seed, N_K=N_K)
    return (c,) + tuple(cases.device_model(rbpf, c))


def _timed_filter(rbpf, c, mdl, x0, P0, Rm):
    """Created, advanced with timing enabled (the distinct-matrix marks are allocated on the first timed step), read out, freed."""
    s = rbpf.FilterSession(mdl, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], Rm, c["N_P"], c["dt"],
                           rng=cases.device_rng(rbpf, c), keep_history=True)
    try:
        during = _live(rbpf)
        s.timing(True)
        s.advance(c["y"].shape[0])
        s.sync()
        timed = _live(rbpf)
        tm = s.timing()
        out = s.finish(want=("traj_max", "traj_mean", "xl_max", "xl_mean", "P_max", "P_mean", "traj_sample_iwmax", "xn_traj",
                             "final_xn", "final_xl", "final_P"))
    finally:
        s.close()
    assert tm["launches"] > 0 and np.all(np.isfinite(out["P_max"]))
    return during, timed


def test_filter_with_timing_returns_every_byte(rbpf):
    base = _live(rbpf)
    case = _mag(rbpf)
    during, timed = _timed_filter(rbpf, *case)
    assert during > base                      # a stub that always answers the same number cannot pass
    assert timed > during                     # the marks and the counter of the timed steps
    assert _live(rbpf) == base


def test_smoothers_return_every_byte(rbpf):
    base = _live(rbpf)
    c, mdl, x0, P0, Rm = _mag(rbpf, N_P=24, N_T=7, m=130, N_K=2)
    args = (mdl.dynModel, mdl.measModel, mdl.dynResNorm, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], Rm, c["N_P"], 2, c["dt"])
    XNK, _, PK = rbpf.particleSmoother(*args, rng=cases.device_rng(rbpf, c))
    assert np.all(np.isfinite(XNK)) and np.all(np.isfinite(PK))
    assert _live(rbpf) == base
    assert rbpf.chol_refresh_in_use(mdl) > 1                                  # the default at nLin = 133: carried factors
    XNK, _, PK = rbpf.particleSmootherInformationForm(*args, rng=cases.device_rng(rbpf, c))
    assert np.all(np.isfinite(XNK)) and np.all(np.isfinite(PK))
    assert _live(rbpf) == base
    XNK, _, PK = rbpf.particleSmootherInformationForm(*args, rng=cases.device_rng(rbpf, c), chol_refresh=1)
    assert np.all(np.isfinite(XNK)) and np.all(np.isfinite(PK))
    assert _live(rbpf) == base


def test_localization_and_predict_return_every_byte(rbpf):
    base = _live(rbpf)
    c = R.loc_case(64, 12, 13, seed=1)
    mp = rbpf.DenseMagMap(rbpf.DenseMagModel(c["NN"], c["L"]), c["mean"], c["V"], c["sigma2"])
    tmax, tmean, ex = rbpf.particleFilterLocalization(mp.dynModel, mp.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["Q"], np.eye(3),
                                                      c["N_P"], c["dt"], rng=rbpf.ReplayRNG(c["U"], c["Z"]), extras=True)
    assert np.all(np.isfinite(tmax)) and ex["first_degenerate_step"] == -1
    assert _live(rbpf) == base
    pos = np.random.RandomState(2).uniform(-1.0, 1.0, (3, 50)) * np.asarray(c["L"])[:, None]
    dE, var, _ = mp.predict(pos)
    assert np.all(np.isfinite(dE)) and np.all(np.isfinite(var))
    assert _live(rbpf) == base


def test_single_rank_sharded_sessions_return_every_byte(rbpf):
    mg = importlib.import_module(rbpf.__name__ + ".multigpu")
    base = _live(rbpf)
    c, mdl, x0, P0, Rm = _mag(rbpf, N_P=32, N_T=9, m=130, N_K=2)
    T = c["y"].shape[0]
    with mg.ShardedFilterSession(mdl, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], Rm, c["N_P"], c["dt"], rng=rbpf.PhiloxRNG(11),
                                 rank=0, world=1, lazy_depth=3, keep_history=True) as s:
        assert _live(rbpf) > base
        s.advance(T)
        out = s.finish(want=("traj_max", "traj_mean", "xl_max", "P_max", "xl_mean", "P_mean", "traj_sample_iwmax"))
    assert np.all(np.isfinite(out["P_max"]))
    assert _live(rbpf) == base
    with mg.ShardedSmootherSession(mdl, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], Rm, c["N_P"], 2, c["dt"], rng=rbpf.PhiloxRNG(9),
                                   rank=0, world=1, lazy_depth=3, chol_refresh=4) as s:
        assert _live(rbpf) > base
        XNK, _, PK = s.run()
    assert np.all(np.isfinite(XNK)) and np.all(np.isfinite(PK))
    assert _live(rbpf) == base


def test_refused_creations_return_every_byte(rbpf):
    """Both refusals come after the context has allocated: the RNG block is checked behind the problem constants, the layout of
    the lazy update behind the particle banks."""
    base = _live(rbpf)
    c, mdl, x0, P0, Rm = _mag(rbpf, N_P=16, N_T=5, m=16, N_K=2)
    r = c["rng"]
    with pytest.raises(rbpf.RBPFError) as ei:                                 # replay RNG without Ufin for a smoother
        rbpf.particleSmoother(mdl.dynModel, mdl.measModel, mdl.dynResNorm, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], Rm,
                              c["N_P"], 2, c["dt"], rng=rbpf.ReplayRNG(r.U, r.Z, None))
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG and "Ufin" in str(ei.value)
    assert _live(rbpf) == base
    with pytest.raises(rbpf.RBPFError) as ei:                                 # nLin = 19: full-square storage has no lazy update there
        rbpf.FilterSession(mdl, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], Rm, c["N_P"], c["dt"],
                           rng=cases.device_rng(rbpf, c), lazy_depth=2)
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "lazy_depth" in str(ei.value)
    assert _live(rbpf) == base


def test_repeated_sessions_do_not_drift(rbpf):
    base = _live(rbpf)
    case = _mag(rbpf, N_P=16, N_T=5, m=130)
    for _ in range(20):
        _timed_filter(rbpf, *case)
        assert _live(rbpf) == base
