"""CPU: the numpy oracle's particleFilter at measurement widths n_y = 2, 4, 5 and 8 with a full R, on the no-noise synthetic
model, against the extended-precision batch posterior (generic_model.batch_posterior) -- the oracle is the reference of
tests/test_gpu_generic_ny.py, and this pins its own agreement with an answer that does not restate the filter.  These tests
pass with or without the device's support of those widths: they establish the yardstick."""
import numpy as np
import pytest

import generic_model as gm
import generic_ny_cases as gc
import rbpf_oracle as O


@pytest.mark.parametrize("shape", sorted(gc.KAT, key=lambda s: s[3]))
def test_oracle_filter_equals_the_long_double_batch_posterior_at_any_width(shape):
    N_P, N_T = 2, gc.KAT[shape]
    m, p, ref = gc.kat_case(shape, N_P, N_T)
    R = p["R"]
    assert R.shape == (shape[3], shape[3]) and np.max(np.abs(R - np.diag(np.diag(R)))) > 1e-4    # R really is full
    out = O.particleFilter(m, p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], R, N_P, p["dt"],
                           O.ReplayRNG(p["U"], p["Z"]), trace=True)
    np.testing.assert_array_equal(out["xn_traj"], np.repeat(gm.path_of(m, p)[:, None, :], N_P, axis=1))
    tr = out["trace"]
    gc.check_kat(ref, p, N_T, lambda i: tr["xl"][:, i], lambda i: tr["P"][:, :, i], lambda i: tr["logw"][:, i], N_P)
