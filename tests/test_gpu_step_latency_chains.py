"""The block-lower step body after its latency chains were shortened: global loads asked for at kernel entry,
K_s' H' formed in front of the tile stream, the innovation statistics on the lanes of one wave, the Jacobian columns rotated by
three.  No floating-point operation changed, so the checks are the project's usual ones (ancestor indices exact, 1e-9 relative
against the numpy oracle), at the places where the new code can go wrong:

  * the jitter retry and the second failure THROUGH the block-lower body (the older jitter tests run the full-square kernel at
    m = 16): the factorisation now runs on every lane of wave 0 and the three logarithms are one call;
  * the column rotation and the prefetch rounds at n = 259 (two column phases, two rounds + 3), 387 (three waves: 2 * 192 + 3),
    515 (the headline) and 639 (127 border rows: the border columns beyond the four that the combine asks for early);
  * N = 1 and N = 3 at m = 512, lazy_depth 4, both bank arrangements;
  * two runs of the same problem agree bit for bit (the sums keep their order whatever the timing of the waves).

Every oracle run is made once and shared."""
import functools

import numpy as np
import pytest

import cases
from test_gpu_filter import check_filter, rel

pytestmark = pytest.mark.gpu
RTOL = 1e-9


def run_sym(rbpf, c, lazy_depth, inplace=0):
    mdl, _, _, _ = cases.device_model(rbpf, c)
    return rbpf.particleFilter(mdl.dynModel, mdl.measModel, c["odometry"], c["y"], c["x0_nonLin"], c["x0_lin"], c["P0_lin"],
                               c["Q"], c["R"], c["N_P"], c["dt"], rng=cases.device_rng(rbpf, c), extras=True,
                               lazy_depth=lazy_depth, inplace=inplace, storage="fp64sym")


@functools.lru_cache(maxsize=None)
def plain_case(N_P, N_T, m, seed):
    c = cases.mag_case(N_P, N_T, m, seed=seed)
    return c, cases.oracle_filter(c)


@functools.lru_cache(maxsize=None)
def jitter_case(m):
    """S = H P H' + R with P0 * 1e-9 and R = -2e-4 I: not positive definite, positive definite with the jitter added."""
    c = cases.mag_case(6, 5, m, seed=12)
    c = dict(c, P0_lin=c["P0_lin"] * 1e-9, R=-2e-4 * np.eye(3))
    return c, cases.oracle_filter(c)


@pytest.mark.parametrize("lazy_depth", [0, 3])
@pytest.mark.parametrize("m", [256, 512])
def test_jitter_retry_through_the_block_lower_body(rbpf, m, lazy_depth):
    """particleFilter.m:145-148 in step_sym_kernel: chol(S) fails at every factorisation, chol(S + jitter I) passes; the
    downdate uses the un-jittered S (:198).  Tolerances as in test_jitter_retry_path_matches_oracle."""
    c, ref = jitter_case(m)
    ex = run_sym(rbpf, c, lazy_depth)[8]
    assert np.all(np.isfinite(ex["w"])) and np.all(np.isfinite(ex["P"]))
    np.testing.assert_array_equal(ex["ai"][1:], ref["trace"]["ai"][1:])
    assert rel(ex["w"], ref["trace"]["w"]) <= RTOL
    assert rel(ex["P"], ref["trace"]["P"]) <= 1e-8
    assert rel(ex["xl"], ref["trace"]["xl"]) <= 1e-8


def test_second_failure_through_the_block_lower_body(rbpf):
    c = cases.mag_case(6, 5, 256, seed=12)
    c = dict(c, P0_lin=c["P0_lin"] * 1e-9, R=-1.0 * np.eye(3))
    with pytest.raises(rbpf.RBPFError) as ei:
        run_sym(rbpf, c, 0)
    assert ei.value.status == rbpf.RBPF_ERR_CHOL_FAILED


@pytest.mark.parametrize("m", [256,      # n = 259: two column phases, two rounds of columns + 3
                               384,      # n = 387: three waves, 2 * 192 + 3
                               512,      # n = 515: the headline size
                               636])     # n = 639: 127 border rows
def test_column_mapping_and_early_loads_at_every_shape(rbpf, m):
    c, ref = plain_case(4, 6, m, 19)
    check_filter(ref, run_sym(rbpf, c, 3))


@pytest.mark.parametrize("inplace", [0, 1])
@pytest.mark.parametrize("N_P", [1, 3])
def test_headline_size_with_one_and_three_particles(rbpf, N_P, inplace):
    c, ref = plain_case(N_P, 6, 512, 19)
    check_filter(ref, run_sym(rbpf, c, 4, inplace=inplace))


def test_two_runs_agree_bit_for_bit(rbpf):
    c = cases.mag_case(8, 11, 512, seed=29)
    a, b = run_sym(rbpf, c, 4), run_sym(rbpf, c, 4)
    for x, y in zip(a[:8], b[:8]):
        np.testing.assert_array_equal(x, y)
    for k in ("ai", "logw", "w", "xl", "P", "xn"):
        np.testing.assert_array_equal(a[8][k], b[8][k])
