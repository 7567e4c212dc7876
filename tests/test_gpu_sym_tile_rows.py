"""GPU: block-lower covariance storage (rbpf_options.storage = 2 / 3) at 6, 10, 12 and 14 tile rows of 64 (nLin 384..511 and
640..1023) -- the runtime-count instantiation of step_sym_kernel (CH = 0, rbpf_step_sym.hip) -- against the numpy oracle on replayed
random numbers, against the full square on the device generator, in the sharded filter, and the refusals of what it leaves out.

Tolerances as in tests/test_gpu_generic_shapes.py: resampling and ancestor indices bit-exact, everything else 1e-9 relative; fp32
tiles 2e-5."""
import importlib

import numpy as np
import pytest

import cases
import test_gpu_generic_shapes as gs
import test_gpu_sharded as sh
import test_gpu_smoother as ts
from test_gpu_filter import check_filter, rel

pytestmark = pytest.mark.gpu
RTOL = 1e-9
COUNTS = (6, 10, 12, 14)


# ---- generic (host-callback) model at every new count, without and with a full 127-row border ---------------------------------
@pytest.fixture(scope="module")
def generic_cases():
    return {}


def _generic(cache, n):
    if n not in cache:
        cache[n] = gs.case((3, 3, 3, 3, n), 8, 6)
    return cache[n]


@pytest.mark.parametrize("lazy_depth,inplace", [(0, -1), (3, -1), (4, -1), (3, 1)])
@pytest.mark.parametrize("border", [0, 127])
@pytest.mark.parametrize("ch", COUNTS)
def test_generic_model_on_block_lower_storage(rbpf, generic_cases, ch, border, lazy_depth, inplace):
    """nLin = 64 CH (no border row) and 64 CH + 127: every (NS, WR) the filter asks for at lazy_depth 0 / 3 / 4, ping-pong banks and
    one bank rewritten in place."""
    gs.filter_parity(rbpf, *_generic(generic_cases, 64 * ch + border), storage="fp64sym", lazy_depth=lazy_depth, inplace=inplace)


@pytest.mark.parametrize("ch", COUNTS)
def test_fp32_tiles(rbpf, generic_cases, ch):
    """fp32 tiles (storage = 3) with a full border: storage precision."""
    gs.fp32_filter_parity(rbpf, *_generic(generic_cases, 64 * ch + 127), storage="fp32sym", lazy_depth=3)


# ---- built-in dense-mag model --------------------------------------------------------------------------------------------------
def _run_mag(rbpf, c, **kw):
    mdl, x0, P0, R = cases.device_model(rbpf, c)
    return rbpf.particleFilter(mdl.dynModel, mdl.measModel, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], R, c["N_P"], c["dt"],
                               rng=cases.device_rng(rbpf, c), extras=True, **kw)


@pytest.mark.parametrize("m", [384, 640, 768, 1000])
def test_dense_mag_filter_matches_oracle(rbpf, m):
    """m = 384, 640, 768 (nLin = m + 3: three border rows) and m = 1000 (nLin 1003: fourteen tile rows and 107 border rows)."""
    c = cases.mag_case(8, 7, m, seed=43)
    check_filter(cases.oracle_filter(c), _run_mag(rbpf, c, storage="fp64sym", lazy_depth=4))


# ---- smoothers at 6 and 10 tile rows ---------------------------------------------------------------------------------------------
def _smooth(rbpf, c, info_form, **kw):
    mdl, x0, P0, R = cases.device_model(rbpf, c)
    f = rbpf.particleSmootherInformationForm if info_form else rbpf.particleSmoother
    return f(mdl.dynModel, mdl.measModel, mdl.dynResNorm, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], R, c["N_P"], c["N_K"],
             c["dt"], rng=cases.device_rng(rbpf, c), extras=True, **kw)


@pytest.mark.parametrize("m", [384, 640])
def test_covariance_form_smoother(rbpf, m):
    c = cases.mag_case(4, 5, m, seed=47, N_K=3)
    ts.check(cases.oracle_smoother(c, False), _smooth(rbpf, c, False, storage="fp64sym"), 3)


@pytest.mark.parametrize("m,chol_refresh", [(384, 5), (384, 1), (640, 0)])
def test_information_form_smoother(rbpf, m, chol_refresh):
    """lazy_depth 3.  Six tile rows: carried factors refreshed every 5th step and the from-scratch factorisation; ten tile rows
    (nLin 643 > 575): the automatic choice is the from-scratch factorisation."""
    lib = rbpf.load_library()
    if chol_refresh == 0:
        assert lib.rbpf_chol_refresh_resolve(1, m + 3, 3, 0) == 1
    c = cases.mag_case(4, 7, m, seed=53, N_K=3)
    ts.check(cases.oracle_smoother(c, True), _smooth(rbpf, c, True, storage="fp64sym", lazy_depth=3, chol_refresh=chol_refresh), 3)


# ---- sharded filter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy_depth", [0, 3])
def test_sharded_filter_at_ten_tile_rows(lazy_depth):
    """World 2 on one GPU at m = 640: without the lazy update bit-identical to the single-GPU block-lower run, with it 1e-9."""
    T, m, n_local = 7, 640, 8
    tm, tx, stats = sh._run(2, "gloo", "host", T, m, n_local, "device", lazy_depth, "fp64sym")
    ref = sh._single(T, m, 2 * n_local, "fp64sym")
    assert stats["steps"] == T
    if lazy_depth == 0:
        np.testing.assert_array_equal(tm, ref["traj_mean"])
        np.testing.assert_array_equal(tx, ref["traj_max"])
    else:
        np.testing.assert_allclose(tm, ref["traj_mean"], rtol=RTOL, atol=1e-11)
        np.testing.assert_allclose(tx, ref["traj_max"], rtol=RTOL, atol=1e-11)


# ---- one larger run on the device generator --------------------------------------------------------------------------------------
def test_twelve_tile_rows_against_the_full_square_on_philox_streams(rbpf):
    """m = 768 (nLin 771), N = 4096, 12 steps, lazy_depth 4, one bank in place: the same resampling indices as the full square,
    outputs to 1e-9, two block-lower runs bit-identical (fixed summation order)."""
    from test_gpu_configs import mag_inputs
    N, steps = 4096, 12
    d, mdl, x0, P0, R = mag_inputs(rbpf, 20, 768)
    want = ("traj_max", "traj_mean", "xl_max", "P_max", "trace_w", "trace_ai", "xl_mean")

    def go(storage):
        with rbpf.FilterSession(mdl, d["dx"], d["y"], d["initState"], x0, P0, cases.Q_MAG, R, N, 0.01, rng=rbpf.PhiloxRNG(5),
                                keep_history=True, trace=True, lazy_depth=4, inplace=1, storage=storage) as s:
            s.advance(steps)
            s.sync()
            assert s.schedule()[0] == 1
            return s.finish(want=want)
    a, a2, full = go("fp64sym"), go("fp64sym"), go("fp64")
    np.testing.assert_array_equal(a["trace_ai"], full["trace_ai"])
    for k in want:
        np.testing.assert_array_equal(a[k], a2[k], err_msg=k)
        if k != "trace_ai":
            sl = (slice(None), slice(0, steps)) if k in ("traj_max", "traj_mean", "trace_w") else Ellipsis
            assert rel(a[k][sl], full[k][sl]) <= RTOL, k


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _refused(rbpf, fn):
    with pytest.raises(rbpf.RBPFError) as ei:
        fn()
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED, ei.value
    return str(ei.value)


@pytest.mark.parametrize("m", [765, 1000])
@pytest.mark.parametrize("info_form", [False, True])
def test_smoothers_at_twelve_and_fourteen_tile_rows_are_refused(rbpf, m, info_form):
    c = cases.mag_case(4, 3, m, seed=59, N_K=2)
    assert "filter only" in _refused(rbpf, lambda: _smooth(rbpf, c, info_form, storage="fp64sym"))


def test_sharded_smoother_at_the_new_counts_is_refused(rbpf):
    mg = importlib.import_module(rbpf.__name__ + ".multigpu")
    c = cases.mag_case(8, 3, 384, seed=61, N_K=2)
    mdl, x0, P0, R = cases.device_model(rbpf, c)
    msg = _refused(rbpf, lambda: mg.ShardedSmootherSession(mdl, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], R, 8, 2, c["dt"],
                                                           rng=cases.device_rng(rbpf, c), rank=0, world=1, transport="host",
                                                           force_collectives=False, storage="fp64sym"))
    assert "sharded smoother" in msg
