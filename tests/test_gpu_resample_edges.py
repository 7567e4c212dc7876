"""Resampling on the device's own weights, with draws placed on the edges of their strict cumsum.

On every production path the running sum the search bisects is a parallel prefix (strips of ceil(N/1024) elements per thread,
a wave scan and wave offsets in normalise_block; 1024-element blocks in rs_weights_kernel / rs_offsets_kernel for N > 8192),
and a draw is taken from it only when a rounding bound certifies that the strict left-to-right cumsum of tools/sample.m:30
decides the same way; one uncertified draw sends the whole step through the strict sum.  These tests shape the step-0
weights through per-particle x0_lin (particleFilter.m:60-61), read the weights the device itself traced, and require

    ai[1] == minimum(sum(cumsum(w0) < u), N - 1)          for EVERY slot

for draws on / one ulp around cdf edges (edge run: exactly one strict recomputation counted) and for draws at a relative
distance >= 1e-9 from every edge (benign run: none counted -- the widest tolerance in the code at N <= 16384 is
1.7e-16 (N + 80) < 3e-12, so the fast path has to be taken).

Weights: at t = 0 every particle has the same x0_nonLin, hence the same H and S = H P0 H' + R.  With x0_lin[:, i] = a_i v,
v = H' / |H|, h = |H|, the log-weight is -(y0 - a_i h)^2 / (2 S) + const, so a_i = (y0 - sqrt(2 S L_i)) / h gives
w_i proportional to exp(-L_i).  After normalisation w_i = exp(-(L_i + ln sum_j exp(-L_j))): exactly 0 from 745.14 on,
denormal from 708.4 on.

Details the pattern rules leave open, and how they are settled here:
  * `plateaus`, strip rule (zeros on every index = 0 and = -1 modulo the strip length S = ceil(N/1024)): at S = 1 and 2 that
    would zero every weight, so there the period is the span of one wave, 64 S.
  * `range`: L = 744 plus the normaliser ln(N/5) >= 5.2 lies beyond 745.14: that class is exactly 0 (N/5 zeros intended);
    the denormal range is reached by L = 720.
  * the edge set holds at most N/4 indices (three draws each have to fit in N slots): the fixed indices and boundaries
    first, then plateau ends (a seeded subsample when there are too many), then seeded random indices.
  * input condition: a CPU model of the device's prefix (same association order, written from the description above)
    differs from the strict cumsum at >= 50 % of the edge set.  It is asserted wherever the surviving weights make the two
    orders round differently, and only printed where they cannot: `dominant` (partial sums of denormals are exact: 0 %),
    `uniform` (k equal weights sum with few roundings in any order: 98-100 % in strip form but 6 % and 14 % in the two
    blocked sizes 8193 and 16384 where w is close to 2^-13 and 2^-14) and `range` at N = 1000 (strip length 1 and only
    the 200 equal top weights survive rounding: 47 %).

Path (iii), search_kernel + resample_fixup_kernel behind normalise_scan_kernel's strip prefix at N <= 8192, is reached by
the smoothers' forward pass (ctx_draw_ancestors).  particleSmootherInformationForm refuses a per-particle x0_lin (quirk Q5:
the reference repmat's a single column), so the weights cannot be shaped there; the covariance-form particleSmoother takes
them, runs the same ctx_draw_ancestors, and its trace exposes step-0 w and step-1 ancestors (iteration 0 draws all N
slots).  rbpf_particle_smoother has no context to read the fallback counter from, so those cases check the indices of
both runs only.

Measured on an MI355X: resample_fallbacks = 1 in the edge run and 0 in the benign run of every one of the 35 filter cases
(each test prints its counts, the number of placed draws and the input-condition fraction).
"""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

SIZES = (1000, 1025, 4097, 8192, 8193, 9217, 16384)
PATTERNS = ("uniform", "plateaus", "lead_trail", "range", "dominant")
M_BASIS = 16
EXP_ZERO = 745.14            # exp(-x) rounds to 0 beyond ln(2^1075) = 745.13
EXP_TINY = 744.44            # ... and to the smallest denormal from ln(2^1074) on: between the two, rounding decides
_case_cache = {}


def strip_len(N):
    return (N + 1023) // 1024


def drops(pattern, N):
    """L [N]: w_i proportional to exp(-L_i)."""
    L = np.zeros(N)
    if pattern == "uniform":
        return L
    if pattern == "plateaus":
        S = strip_len(N)
        period = S if S >= 3 else 64 * S
        idx = np.arange(N)
        L[(idx % period == 0) | (idx % period == period - 1)] = 800.0
        for b in (64, 1024, 2048):
            if b < N:
                L[b - 1:b + 1] = 800.0
        L[N // 2 - 150:N // 2 + 150] = 800.0
        return L
    if pattern == "lead_trail":
        K = 1500 if N >= 4000 else N // 4
        L[:K] = 800.0
        L[N - K:] = 800.0
        return L
    if pattern == "range":
        return np.array([0.0, 40.0, 200.0, 720.0, 744.0])[np.arange(N) % 5]
    if pattern == "dominant":
        L[:] = 730.0
        L[N - 2] = 0.0
        return L
    raise ValueError(pattern)


def intended_zeros(L):
    """Entries whose normalised weight exp(-(L_i + ln sum exp(-L))) is exactly 0; no entry may sit where rounding decides."""
    z = L + np.log(np.sum(np.exp(-L)))
    assert not np.any((z > EXP_TINY - 0.5) & (z < EXP_ZERO + 0.5)), "a drop in the band where exp's rounding decides"
    return z > EXP_ZERO


def problem(N, seed=21):
    if N not in _case_cache:
        c = cases.radio_case(N, 2, M_BASIS, seed=seed)
        H = np.asarray(c["model"].measModel(c["x0_nonLin"]), dtype=np.float64).reshape(-1)
        h = float(np.linalg.norm(H))
        S = float(H @ c["P0_lin"] @ H + c["R"][0, 0])
        assert h > 0.1 and S > 0
        _case_cache[N] = dict(c=c, v=H / h, h=h, S=S, y0=float(np.ravel(c["y"])[0]))
    return _case_cache[N]


def x0_lin_for(p, L):
    a = (p["y0"] - np.sqrt(2.0 * p["S"] * L)) / p["h"]
    return np.outer(p["v"], a)                                  # [nLin x N_P]


def run_filter(rbpf, p, x0, U):
    c = p["c"]
    mdl, _, P0, R = cases.device_model(rbpf, c)
    rng = rbpf.ReplayRNG(U, c["rng"].Z, c["rng"].Ufin)
    out = rbpf.particleFilter(mdl.dynModel, mdl.measModel, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], R, c["N_P"],
                              c["dt"], rng=rng, extras=True)
    ex = out[8]
    return ex["w"][0].copy(), ex["ai"][1].copy(), ex["resample_fallbacks"]


def run_smoother(rbpf, p, x0, U):
    c = p["c"]
    mdl, _, P0, R = cases.device_model(rbpf, c)
    rng = rbpf.ReplayRNG(U, c["rng"].Z, c["rng"].Ufin)
    out = rbpf.particleSmoother(mdl.dynModel, mdl.measModel, mdl.dynResNorm, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], R,
                                c["N_P"], 1, c["dt"], rng=rng, extras=True)
    ex = out[3]
    return ex["w"][0, 0].copy(), ex["ai"][0, 1].copy(), None


def hillis_steele_64(x):
    """Inclusive scan of every row of x [waves x 64] in the order of a wave scan: inc[l] += inc[l - off], off = 1, 2, .., 32."""
    inc = x.copy()
    for off in (1, 2, 4, 8, 16, 32):
        nxt = inc.copy()
        nxt[:, off:] = inc[:, off:] + inc[:, :-off]
        inc = nxt
    return inc


def block_prefix_1024(v):
    """Inclusive prefix of v [1024] the way one 1024-thread block forms it: wave scans, then the wave totals added in order."""
    inc = hillis_steele_64(v.reshape(16, 64))
    woff = np.concatenate(([0.0], np.cumsum(inc[:-1, 63])))
    return (woff[:, None] + inc).reshape(-1)


def device_shaped_prefix(w, blocked):
    """The parallel prefix in the device's association order (CPU model for the input condition; additions only, so IEEE
    doubles reproduce it).  blocked: 1024-element blocks + block offsets in order (N > 8192 in the filter); else strips."""
    N = w.size
    if blocked:
        B = (N + 1023) // 1024
        lp = np.concatenate([block_prefix_1024(b) for b in np.pad(w, (0, B * 1024 - N)).reshape(B, 1024)])
        soff = np.concatenate(([0.0], np.cumsum(lp[1023::1024])))[:B]
        out = lp.reshape(B, 1024).copy()
        out[1:] = soff[1:, None] + out[1:]
        return out.reshape(-1)[:N]
    S = strip_len(N)
    strips = np.pad(w, (0, 1024 * S - N)).reshape(1024, S)
    tot = np.zeros(1024)
    for k in range(S):
        tot = tot + strips[:, k]
    incw = hillis_steele_64(tot.reshape(16, 64))               # wave scan of the strip totals
    exc = np.concatenate((np.zeros((16, 1)), incw[:, :-1]), axis=1)
    woff = np.concatenate(([0.0], np.cumsum(incw[:-1, 63])))   # wave totals added in order
    run = (woff[:, None] + exc).reshape(-1)                    # what thread tid starts its strip from
    out = np.empty((1024, S))
    for k in range(S):
        run = run + strips[:, k]
        out[:, k] = run
    return out.reshape(-1)[:N]


def zero_runs(w):
    z = np.concatenate(([0], (w == 0).astype(np.int8), [0]))
    d = np.diff(z)
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1          # first and last index of every run


def edge_set(w0, rs):
    N = w0.size
    S = strip_len(N)
    first = [0, 1, N - 2, N - 1]
    for b in [64, 1024, 2048, N // 2 - 150, N // 2 + 150] + list(range(1024, N, 1024)) + list(range(64 * S, N, 64 * S)):
        first += [b - 1, b]
    first = [j for j in dict.fromkeys(first) if 0 <= j < N]
    cap = N // 4
    a, b = zero_runs(w0)
    ends = np.unique(np.concatenate((a, b, np.maximum(a - 1, 0), np.minimum(b + 1, N - 1))))
    ends = np.setdiff1d(ends, first)
    room = max(cap - len(first), 0)
    if ends.size > room // 2:
        ends = rs.choice(ends, room // 2, replace=False)
    E = np.unique(np.concatenate((np.array(first[:cap], dtype=np.int64), ends.astype(np.int64))))
    rest = np.setdiff1d(np.arange(N), E)
    E = np.unique(np.concatenate((E, rs.choice(rest, cap - E.size, replace=False))))
    assert E.size == cap
    return E


def edge_draws(wc, E, rs):
    N = wc.size
    vals = np.concatenate((wc[E], np.nextafter(wc[E], 2.0), np.nextafter(wc[E], -1.0)))
    vals = vals[(vals > 0.0) & (vals <= 1.0)]
    vals = np.concatenate((vals, [np.nextafter(0.0, 1.0), 1.0 - 2.0 ** -53]))
    assert vals.size <= N
    u = rs.random_sample(N)
    u[rs.permutation(N)[:vals.size]] = vals
    return u, vals.size


def edge_distance(wc, u):
    """Smallest relative distance of every u to an entry of the (non-decreasing) wc."""
    k = np.searchsorted(wc, u)
    lo, hi = wc[np.clip(k - 1, 0, wc.size - 1)], wc[np.clip(k, 0, wc.size - 1)]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.minimum(np.abs(u - lo) / np.maximum(u, lo), np.abs(u - hi) / np.maximum(u, hi))
    return d


def benign_draws(wc, rs):
    u = rs.random_sample(wc.size)
    for _ in range(20):
        bad = edge_distance(wc, u) < 1e-9
        if not bad.any():
            break
        u[bad] = rs.random_sample(int(bad.sum()))
    assert np.all(edge_distance(wc, u) >= 1e-9) and np.all((u > 0) & (u < 1))
    return u


def strict_indices(wc, u):
    return np.minimum(np.searchsorted(wc, u, side="left"), wc.size - 1).astype(np.int64)     # sum(wc < u): wc is non-decreasing


def check_case(rbpf, run, N, pattern, blocked, want_counts, need_half):
    p = problem(N)
    L = drops(pattern, N)
    zero = intended_zeros(L)
    assert (~zero).sum() >= 1
    x0 = x0_lin_for(p, L)
    U0 = p["c"]["rng"].U
    assert U0.shape == (1, 1, N)
    w0, _, _ = run(rbpf, p, x0, U0)
    # the pattern did not degenerate on the device
    assert np.all(np.isfinite(w0)) and np.all(w0 >= 0) and abs(w0.sum() - 1.0) < 1e-9
    np.testing.assert_array_equal(w0 == 0, zero)
    wc = np.cumsum(w0)
    assert np.all(np.diff(wc) >= 0)
    if pattern == "uniform":
        assert np.all(w0 == w0[0])
    if pattern == "range":
        assert np.sum((wc[1:] == wc[:-1]) & (w0[1:] > 0)) >= N / 10
        assert np.any((w0 > 0) & (w0 < 2.3e-308))                         # denormal weights are present
    if pattern == "dominant":
        assert int(np.argmax(w0)) == N - 2 and w0[N - 2] > 0.99 and np.all(np.delete(w0, N - 2) < 2.3e-308)
    rs = np.random.RandomState(1000 + N)
    E = edge_set(w0, rs)
    frac = float(np.mean(device_shaped_prefix(w0, blocked)[E] != wc[E]))
    print(f"N={N} {pattern}: device-shaped prefix != strict cumsum on {100 * frac:.1f} % of {E.size} edge indices")
    if need_half:
        assert frac >= 0.5
    # edge run
    u, n_edge = edge_draws(wc, E, rs)
    w1, ai, nfb = run(rbpf, p, x0, u[None, None, :])
    np.testing.assert_array_equal(w1, w0)
    np.testing.assert_array_equal(ai, strict_indices(wc, u))
    print(f"N={N} {pattern}: edge run {n_edge} placed draws, fallbacks {nfb}")
    if want_counts:
        assert nfb == 1
    # benign run
    u = benign_draws(wc, rs)
    w2, ai, nfb = run(rbpf, p, x0, u[None, None, :])
    np.testing.assert_array_equal(w2, w0)
    np.testing.assert_array_equal(ai, strict_indices(wc, u))
    print(f"N={N} {pattern}: benign run fallbacks {nfb}")
    if want_counts:
        assert nfb == 0


def rounding_expected(N, pattern):
    """Where the >= 50 % input condition is asserted (see the module docstring)."""
    return pattern in ("plateaus", "lead_trail") or (pattern == "range" and N != 1000)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N", SIZES)
def test_filter_draws_on_the_edges_of_its_own_weights(rbpf, N, pattern):
    """(i) the fused normalise_resample_kernel / search_block up to N = 8192, (ii) search_kernel + resample_fixup_kernel behind
    the multi-workgroup prefix above."""
    check_case(rbpf, run_filter, N, pattern, blocked=N > 8192, want_counts=True, need_half=rounding_expected(N, pattern))


@pytest.mark.parametrize("pattern", ("plateaus", "range"))
@pytest.mark.parametrize("N", (1025, 8192))
def test_smoother_forward_pass_draws_on_the_edges_of_its_own_weights(rbpf, N, pattern):
    """(iii) ctx_draw_ancestors: search_kernel + resample_fixup_kernel behind normalise_scan_kernel's strip prefix."""
    check_case(rbpf, run_smoother, N, pattern, blocked=False, want_counts=False, need_half=True)


def test_session_counter_counts_flagged_steps_only(rbpf):
    """FilterSession.resample_fallbacks(): 0 before any step, 1 after a step with one draw exactly on a cdf edge (every other
    draw benign), unchanged by a reset, 2 after the same step again."""
    N = 1025
    p = problem(N)
    c = p["c"]
    x0 = x0_lin_for(p, drops("plateaus", N))
    w0, _, _ = run_filter(rbpf, p, x0, c["rng"].U)
    wc = np.cumsum(w0)
    rs = np.random.RandomState(5)
    u = benign_draws(wc, rs)
    u[700] = wc[N // 3]
    assert w0[N // 3] > 0
    mdl, _, P0, R = cases.device_model(rbpf, c)
    rng = rbpf.ReplayRNG(u[None, None, :], c["rng"].Z, c["rng"].Ufin)
    with rbpf.FilterSession(mdl, c["odometry"], c["y"], c["x0_nonLin"], x0, P0, c["Q"], R, N, c["dt"], rng=rng) as s:
        assert s.resample_fallbacks() == 0
        s.advance(2)
        assert s.resample_fallbacks() == 1
        s.reset()
        assert s.resample_fallbacks() == 1
        s.advance(2)
        assert s.resample_fallbacks() == 2
