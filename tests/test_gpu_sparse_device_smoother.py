"""GPU: the covariance-form smoother's sparseFeatures = true branch (src/particleSmoother.m:194-217,267-277,306-321) with
arbitrary models whose handles are device code -- rbpf.DeviceSparseSmootherHandles, rbpf_particle_smoother_sparse_device -- against
oracle/rbpf_oracle.py:particleSmoother(model, ..., sparseFeatures=True).  The numpy side of every model is in
tests/sparse_models.py (the pinhole camera: the oracle's own SparseVisualModel), its torch twin in
tests/sparse_models_torch_smoother.py.  The standard is tests/test_gpu_sparse.py:check_smoother's: ak and every ancestor index
exact (the reference slot's included), w, paNt, XNK, XLK and PK within 1e-9.

Seeds.  "Indices exact" needs every uniform to stay clear of the cdf edges of the distribution it samples, so for every case
the smallest distance between any uniform used (ordinary ancestors, the reference slot's ancestor, ak) and those edges was computed
from the oracle's trace on the CPU; every case below keeps at least 1e-7:

    case                                       problem seed / rng seed     margin
    pinhole (8, 9, 5), N_K = 3                 6 / 306                      3.8e-05
    pinhole (10, 12, 20), N_K = 3              6 / 306                      4.0e-05
    range-bearing L = 3, N_P = 7, N_T = 8      3 / 503                      9.0e-04
    range-bearing L = 16, N_P = 9, N_T = 6     3 / 503                      4.5e-04
    range-only (32, 96), N_P = 5, N_T = 4      4 / 604                      3.8e-03
    patterns (range-bearing 3, 7, 6)           7 / 507                      4.8e-04
    jitter (range-bearing 3, 6, 5)             12 / 512                     1.1e-03

The jitter case: with P0_lin * 1e-9 and R = -2e-4 I the oracle (jitter 1e-2, :70) finishes without CholeskyFailure and takes the
retry in every one of its 48 ancestor-weight factorisations (M = 19, 15, 12, 6), counted on the CPU by wrapping
rbpf_oracle._chol_lower_with_jitter and looking at its caller."""
import functools
import importlib

import numpy as np
import pytest

import cases
import rbpf_oracle as O
import sparse_models as sm
from test_gpu_sparse import RTOL, check_smoother, rel, run_smoother

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _device():
    torch = _torch()
    return torch.device("cuda", torch.cuda.current_device())


def _twin(c, **kw):
    smts = importlib.import_module("sparse_models_torch_smoother")
    return smts.twin_of(c["model"], c, _device(), **kw)


def _args(c):
    return (c["odometry"], c["y"], c["x0_nonLin"], c["x0_lin"], c["P0_lin"], c["Q"], c["R"], c["N_P"], c["N_K"], c["dt"])


def run(rbpf, c, twin=None, future_chunk=None, drn=False, **kw):
    tw = twin if twin is not None else _twin(c)
    h = rbpf.DeviceSparseSmootherHandles(tw.dynModel, tw.measModel, tw.dynResNorm if drn else None, future_chunk)
    return rbpf.particleSmoother(h, None, None, *_args(c), True, rng=cases.device_rng(rbpf, c), extras=True, **kw)


def smoother_case(c, N_K, seed):
    """range_bearing_case / range_only_case draw their ReplayRNG for N_K = 1: the smoother's has N_K pages."""
    return dict(c, rng=O.ReplayRNG.draw(seed, N_K, c["y"].shape[0], c["N_P"], 3), N_K=N_K)


def patterns_problem():
    """The last step entirely NaN (M = 0 at t = N_T - 1), one step in the middle entirely NaN (a skipped future time) and one
    output never observed at any time."""
    c = sm.range_bearing_case(3, 7, 6, seed=7)
    y = c["y"].copy()
    y[-1, :] = np.nan
    y[3, :] = np.nan
    y[:, 4] = np.nan
    return dict(c, y=y)


@functools.lru_cache(maxsize=None)
def case(name):
    """(problem, oracle result), computed once and shared."""
    kind, *a = name.split(":")
    a = [int(v) for v in a]
    if kind == "pinhole":
        c = cases.sparse_case(a[0], a[1], a[2], seed=6, N_K=3)
    elif kind == "rb":
        c = smoother_case(sm.range_bearing_case(a[0], a[1], a[2], seed=3), 3, 503)
    elif kind == "ro":
        c = smoother_case(sm.range_only_case(a[0], a[1], a[2], seed=4), 2, 604)
    elif kind == "patterns":
        c = smoother_case(patterns_problem(), 3, 507)
    elif kind == "jitter":
        c = sm.range_bearing_case(3, 6, 5, seed=12)
        c = smoother_case(dict(c, P0_lin=c["P0_lin"] * 1e-9, R=-2e-4 * np.eye(6)), 3, 512)
    return c, cases.oracle_smoother(c, False)


def future_counts(c):
    """M(t), t = 1 .. N_T - 1: the observed outputs of the times t .. N_T - 1."""
    seen = ~np.isnan(c["y"])
    return [int(seen[t:].sum()) for t in range(1, seen.shape[0])]


def assert_same(a, b):
    """Two runs of the product, bit for bit: the three outputs and every trace."""
    for k in range(3):
        np.testing.assert_array_equal(a[k], b[k])
    for key in a[3]:
        np.testing.assert_array_equal(a[3][key], b[3][key], err_msg=key)


# ---- 1. the pinhole twin against the oracle's own model, and against the built-in family -----------------------------------
@pytest.mark.parametrize("N_P,N_T,nLand", [(8, 9, 5), (10, 12, 20)])
def test_pinhole_twin_matches_oracle_and_the_built_in_family(rbpf, N_P, N_T, nLand):
    c, ref = case(f"pinhole:{N_P}:{N_T}:{nLand}")
    out = run(rbpf, c)
    check_smoother(ref, out, 3)
    XNK, XLK, PK, ex = run_smoother(rbpf, c)                                   # SparseVisualModel: sparse_anc_kernel
    np.testing.assert_array_equal(out[3]["ak"], ex["ak"])
    np.testing.assert_array_equal(out[3]["ai"][:, 1:], ex["ai"][:, 1:])
    assert rel(out[0], XNK) <= RTOL and rel(out[1], XLK) <= RTOL and rel(out[2], PK) <= RTOL
    assert rel(out[3]["w"], ex["w"]) <= RTOL
    a, b = out[3]["paNt"][1:, 1:], ex["paNt"][1:, 1:]
    assert np.max(np.abs(a - b)) <= RTOL * max(1.0, np.max(np.abs(b)))


# ---- 2. range-bearing landmarks with the dense coupling: no zero in the Jacobian ---------------------------------------------
@pytest.mark.parametrize("L,N_P,N_T", [(3, 7, 8), (16, 9, 6)])
def test_range_bearing_matches_oracle(rbpf, L, N_P, N_T):
    c, ref = case(f"rb:{L}:{N_P}:{N_T}")
    assert np.all(c["model"].measModel(c["x0_nonLin"], c["x0_lin"][:, 0])[1] != 0.0)
    Ms = set(future_counts(c))
    assert any(m % 16 for m in Ms) and any(m % 4 for m in Ms), Ms              # edges of the 16-row tiles and of the 4-deep k groups
    if L == 3:
        assert 0 < min(Ms) <= 3, Ms                                            # ... and a matrix smaller than one k group
    check_smoother(ref, run(rbpf, c), 3)


# ---- 3. range-only 3-D beacons at the largest admitted shape -------------------------------------------------------------------
def test_range_only_at_the_largest_shape_matches_oracle(rbpf):
    c, ref = case("ro:32:5:4")
    assert c["model"].ny == 32 and c["model"].nLin == 96 and c["N_K"] == 2
    check_smoother(ref, run(rbpf, c), 2)


# ---- 4. observation patterns ---------------------------------------------------------------------------------------------------
def test_observation_patterns_match_oracle(rbpf):
    c, ref = case("patterns")
    seen = ~np.isnan(c["y"])
    assert not seen[-1].any() and not seen[3].any() and not seen[:, 4].any() and seen[2].any() and seen[4].any()
    assert future_counts(c)[-1] == 0
    out = run(rbpf, c)
    check_smoother(ref, out, 3)
    # t = N_T - 1: no future observation, logwMeas = 0 -- the ancestor probabilities are those of the weights and the dynamics
    # alone, and so they are in the oracle
    assert np.all(np.isfinite(out[3]["paNt"][1:, -1]))
    # a twin that writes NaN into the never-observed output's rows of yhat and dy: the same bits
    assert_same(out, run(rbpf, c, twin=_twin(c, nan_rows=(4,))))


# ---- 5. chunking ---------------------------------------------------------------------------------------------------------------
def expected_meas_columns(c, chunk):
    """The column counts of every measModel call of a run: the binding's one call for the layouts (N_P), then per iteration and
    step the chunks of the observed future times (k >= 1, t >= 1) followed by the step's own call."""
    N, K = c["N_P"], c["N_K"]
    seen = (~np.isnan(c["y"])).any(axis=1)
    T = seen.size
    cols = [N]
    for k in range(K):
        for t in range(T):
            if k > 0 and t > 0:
                left = int(seen[t:].sum())
                while left > 0:
                    cols.append(min(chunk, left) * N)
                    left -= min(chunk, left)
            cols.append(N)
    return cols


@pytest.mark.parametrize("name", ["rb:3:7:8", "patterns"])
def test_chunking_is_bit_identical_and_really_chunks(rbpf, name):
    c, ref = case(name)
    T = c["y"].shape[0]
    outs = {}
    for chunk in (1, 2, None):
        tw = _twin(c)
        outs[chunk] = run(rbpf, c, twin=tw, future_chunk=chunk)
        assert tw.columns("meas") == expected_meas_columns(c, chunk if chunk is not None else T), chunk
        assert tw.columns("dyn") == [c["N_P"]] * (T - 1) + [c["N_P"] - 1] * ((T - 1) * (c["N_K"] - 1))
    assert_same(outs[1], outs[None])
    assert_same(outs[2], outs[None])
    check_smoother(ref, outs[1], c["N_K"])
    if name == "patterns":                                                     # chunk = 1: N_T - t calls at step t, minus the skipped times
        seen = (~np.isnan(c["y"])).any(axis=1)
        assert int(seen[1:].sum()) < T - 1


# ---- 6. layouts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dy_mode,yhat_mode", [("matlab", "c"), ("slice", "c"), ("c", "t"), ("matlab", "t"), ("slice", "t")])
def test_layouts_are_bit_identical(rbpf, dy_mode, yhat_mode):
    c, ref = case("rb:3:7:8")
    tw = _twin(c, dy_mode=dy_mode, yhat_mode=yhat_mode)
    torch = _torch()
    for C_ in (c["N_P"], 3 * c["N_P"]):
        xl = torch.zeros(C_, 6, dtype=torch.float64, device=_device()) + 5.0
        yhat, dy = tw.measModel(torch.zeros(3, C_, dtype=torch.float64, device=_device()), xl)
        d = 6
        assert dy.stride() == {"c": (d * d, d, 1), "matlab": (1, C_, C_ * d), "slice": (d * (d + 3), d + 3, 1)}[dy_mode]   # (nLin = n_y here)
        assert yhat.stride() == ((1, C_) if yhat_mode == "t" else (d, 1))
    tw.reset()
    out = run(rbpf, c, twin=tw, future_chunk=3)
    assert_same(out, run(rbpf, c, future_chunk=3))
    check_smoother(ref, out, 3)


# ---- 7. a dynResNorm handle against the additive default -------------------------------------------------------------------------
def test_dyn_res_norm_handle_matches_the_default(rbpf):
    c, ref = case("rb:3:7:8")
    tw = _twin(c)
    with_handle = run(rbpf, c, twin=tw, drn=True)
    assert tw.columns("drn") == [c["N_P"]] * ((c["y"].shape[0] - 1) * (c["N_K"] - 1))
    default = run(rbpf, c)
    check_smoother(ref, with_handle, 3)
    check_smoother(ref, default, 3)
    np.testing.assert_array_equal(with_handle[3]["ak"], default[3]["ak"])
    np.testing.assert_array_equal(with_handle[3]["ai"], default[3]["ai"])
    for k in range(3):
        assert rel(with_handle[k], default[k]) <= RTOL
    a, b = with_handle[3]["paNt"][1:, 1:], default[3]["paNt"][1:, 1:]
    assert np.max(np.abs(a - b)) <= RTOL * max(1.0, np.max(np.abs(b)))


# ---- 8. jitter retry in the ancestor weights ---------------------------------------------------------------------------------------
def test_jitter_retry_in_the_ancestor_weights_matches_oracle(rbpf):
    """S = D P D' + blkdiag(R(ind,ind)) not positive definite on the first try in every ancestor-weight factorisation ->
    chol(S + 1e-2 I) (particleSmoother.m:221-224), and the same in the steps (:70).  Tolerances of the filter's jitter test: 1e-8 on
    P and xl, everything else the standard."""
    c, ref = case("jitter")
    XNK, XLK, PK, ex = run(rbpf, c)
    tr = ref["trace"]
    np.testing.assert_array_equal(ex["ak"], tr["ak"])
    np.testing.assert_array_equal(ex["ai"][:, 1:], tr["ai"][:, 1:])
    assert rel(ex["w"], tr["w"]) <= RTOL
    for k in range(1, 3):
        a, b = ex["paNt"][k, 1:], tr["paNt"][k, 1:]
        assert np.max(np.abs(a - b)) <= RTOL * max(1.0, np.max(np.abs(b)))
    assert rel(XNK, ref["XNK"]) <= RTOL
    assert rel(PK, ref["PK"]) <= 1e-8 and rel(XLK, ref["XLK"]) <= 1e-8


# ---- 9. refusals leave nothing behind ----------------------------------------------------------------------------------------------
def _never(*a):
    raise AssertionError("a refused run called a handle")


def _raises_in_an_ancestor_weight_call(tw, C_):
    def meas(xn, xl):
        if xn.shape[1] == C_:
            raise RuntimeError("boom in measModel")
        return tw.measModel(xn, xl)
    return meas


def _wrong_shape_in_an_ancestor_weight_call(tw, C_):
    def meas(xn, xl):
        out = tw.measModel(xn, xl)
        return tuple(v[:-1] for v in out) if xn.shape[1] == C_ else out
    return meas


def _float32(tw):
    return lambda xn, xl: tuple(v.float() for v in tw.measModel(xn, xl))


REFUSALS = {
    # name: (keywords, status, words of the message)
    "n_devices=2": (dict(n_devices=2), "RBPF_ERR_UNSUPPORTED", "n_devices"),
    "fp32": (dict(storage="fp32"), "RBPF_ERR_UNSUPPORTED", "storage"),
    "lazy_depth=2": (dict(lazy_depth=2), "RBPF_ERR_UNSUPPORTED", "lazy_depth"),
    "inplace=1": (dict(inplace=1), "RBPF_ERR_UNSUPPORTED", "inplace"),
}


@pytest.mark.parametrize("name", list(REFUSALS) + ["M>1023", "information form", "sparseFeatures=False", "raises", "wrong shape", "float32"])
def test_refusals_leave_nothing_behind(rbpf, name):
    c, ref = case("rb:3:7:8")
    lib = rbpf.load_library()
    good = run(rbpf, c, future_chunk=2)
    _torch().cuda.synchronize()
    base = int(lib.rbpf_device_bytes_live())
    tw = _twin(c)
    N = c["N_P"]
    handles = rbpf.DeviceSparseSmootherHandles(tw.dynModel, tw.measModel, None, 2)
    rng = cases.device_rng(rbpf, c)
    if name in REFUSALS:
        kw, status, words = REFUSALS[name]
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleSmoother(handles, None, None, *_args(c), True, rng=rng, **kw)
        assert ei.value.status == getattr(rbpf, status) and words in str(ei.value), str(ei.value)
        assert tw.log == []
    elif name == "M>1023":                                                     # 40 steps x 32 outputs, all observed: M(1) = 1248
        big = (np.zeros((39, 3)), np.zeros((40, 32)), np.zeros(3), np.zeros(64), np.eye(64), 0.01 * np.eye(3), np.eye(32), 4, 2, 1.0)
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleSmoother(rbpf.DeviceSparseSmootherHandles(_never, _never), None, None, *big, True, rng=rbpf.PhiloxRNG(1))
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "more than 1023 future observations" in str(ei.value)
    elif name == "information form":
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleSmootherInformationForm(handles, None, None, *_args(c), True, rng=rng)
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "particleSmoother" in str(ei.value)
        assert tw.log == []
    elif name == "sparseFeatures=False":
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleSmoother(handles, None, None, *_args(c), False, rng=rng)
        assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG and "sparseFeatures" in str(ei.value)
        assert tw.log == []
    else:
        meas, exc, words = {"raises": (_raises_in_an_ancestor_weight_call(tw, 2 * N), RuntimeError, "boom in measModel"),
                            "wrong shape": (_wrong_shape_in_an_ancestor_weight_call(tw, 2 * N), ValueError, "expected a float64 device tensor of shape"),
                            "float32": (_float32(tw), ValueError, "torch.float32")}[name]
        with pytest.raises(exc, match=words):
            rbpf.particleSmoother(rbpf.DeviceSparseSmootherHandles(tw.dynModel, meas, None, 2), None, None, *_args(c), True, rng=rng)
        if name != "float32":                          # it got as far as the first ancestor weights: iteration 1, step 1, and no further
            assert tw.columns("dyn") == [N] * (c["y"].shape[0] - 1) + [N - 1]
            assert (2 * N in tw.columns("meas")) == (name == "wrong shape")    # (the raising wrapper never reaches the twin)
    _torch().cuda.synchronize()
    assert int(lib.rbpf_device_bytes_live()) == base
    assert_same(run(rbpf, c, future_chunk=2), good)                            # a valid run afterwards
    assert int(lib.rbpf_device_bytes_live()) == base


# ---- 10. the filter takes the new object ---------------------------------------------------------------------------------------------
def test_the_filter_takes_the_new_object(rbpf):
    c = sm.range_bearing_case(3, 7, 8, seed=3)
    smt = importlib.import_module("sparse_models_torch")
    a = (c["odometry"], c["y"], c["x0_nonLin"], c["x0_lin"], c["P0_lin"], c["Q"], c["R"], c["N_P"], c["dt"])
    outs = []
    for cls in (rbpf.DeviceSparseSmootherHandles, rbpf.DeviceSparseHandles):
        tw = smt.twin_of(c["model"], c, _device())
        outs.append(rbpf.particleFilter(cls(tw.dynModel, tw.measModel), None, *a, True, rng=cases.device_rng(rbpf, c), extras=True))
    for k in range(8):
        np.testing.assert_array_equal(outs[0][k], outs[1][k])
    for key in outs[1][8]:
        np.testing.assert_array_equal(outs[0][8][key], outs[1][8][key], err_msg=key)


# ---- 11. the build kernel alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,M,N", [(1, 1, 2), (6, 15, 2), (9, 17, 2), (40, 33, 2), (96, 64, 2), (96, 250, 3)])
def test_build_kernel_alone(rbpf, n, M, N):
    """S = D P D' + RS on random symmetric positive definite P, dense random D and a pair table with ragged times, against numpy.
    Per entry |error| <= gamma (|D| |P| |D|')_ab + eps |RS_ab| with gamma = (2 n + 2) eps / (1 - (2 n + 2) eps): the standard bound of
    two chained dot products of length n (n products and n - 1 additions each, one more addition for RS) -- derived, not measured;
    any summation order meets it."""
    torch = _torch()
    rs = np.random.RandomState(100 * n + M)
    d = 5
    A = rs.standard_normal((N, n, n))
    P = A @ np.transpose(A, (0, 2, 1)) + n * np.eye(n)
    D = rs.standard_normal((N, M, n))
    pair_t = np.sort(rs.randint(0, max(M // 3, 1) + 1, M)).astype(np.int32)    # ragged: 0 .. 5 rows per time
    pair_j = rs.randint(0, d, M).astype(np.int32)
    B = rs.standard_normal((d, d))
    R = B @ B.T + np.eye(d)
    RS = np.where(pair_t[:, None] == pair_t[None, :], R[np.ix_(pair_j, pair_j)], 0.0)
    dev = _device()
    S, _ms = rbpf.sparse_ext_build_probe(torch.as_tensor(P, device=dev), torch.as_tensor(D, device=dev), torch.as_tensor(pair_t, device=dev),
                                         torch.as_tensor(pair_j, device=dev), torch.as_tensor(R, device=dev))
    S = S.cpu().numpy()
    eps = np.finfo(np.float64).eps
    gamma = (2 * n + 2) * eps / (1.0 - (2 * n + 2) * eps)
    tiles = np.arange(M) // 16
    read = tiles[:, None] >= tiles[None, :]                                    # the 16 x 16 tiles on and below the diagonal
    for i in range(N):
        want = D[i] @ P[i] @ D[i].T + RS
        bound = gamma * (np.abs(D[i]) @ np.abs(P[i]) @ np.abs(D[i]).T) + eps * np.abs(RS)
        err = np.abs(S[i] - want)
        assert np.all(np.isfinite(S[i][read]))
        worst = np.max((err / bound)[read])
        print(f"n={n} M={M} particle {i}: worst error / bound = {worst:.3g}")
        assert worst <= 1.0
        assert np.all(np.isnan(S[i][~read]))                                   # nothing above them is written
