"""GPU: the pack-and-whiten kernel of the refreshes with device handles (rbpf_ext_pack_whiten_probe): G = W H written from
measModel's layout straight to its place, against the pack kernel followed by the whitening kernel -- the same bits -- and
against numpy within the rounding bound of the fma chain.

Shapes: rows and nLin on, just below, just above and twice past the 64-wide tiles (and the 32-particle tiles of the fused
kernel), one row, one coefficient; n_y = 1 and 3; MATLAB order and C-contiguous."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 65, 130)
NLIN = (1, 63, 64, 65, 130)


def _inputs(rows, d, n):
    rs = np.random.RandomState(rows * 1000 + d * 100 + n)
    return rs.standard_normal((rows, d, n)), rs.standard_normal((d, d))           # a non-symmetric W


@pytest.mark.parametrize("layout", [0, 2])
@pytest.mark.parametrize("d", [1, 3])
def test_fused_equals_pack_then_whiten_bit_for_bit_and_numpy_within_the_fma_bound(rbpf, d, layout):
    for rows in ROWS:
        for n in NLIN:
            dy, W = _inputs(rows, d, n)
            fused = rbpf.pack_whiten_probe(dy, W, dy_layout=layout, fused=True)
            two = rbpf.pack_whiten_probe(dy, W, dy_layout=layout, fused=False)
            np.testing.assert_array_equal(fused, two, err_msg=str((rows, n)))
            # a d-term fma chain: each of its d roundings is relative to a partial sum bounded by sum_b |W_ab| |H_bc|.  The
            # product it is held against is numpy's in long double: an fp64 product carries d roundings of its own, and two
            # results that each keep the bound may differ by twice as much
            want = np.einsum("ab,ibc->iac", W.astype(np.longdouble), dy.astype(np.longdouble))
            bound = d * 2.0 ** -53 * np.einsum("ab,ibc->iac", np.abs(W), np.abs(dy))
            for got in (fused, two):
                assert np.all(np.abs(got - want) <= bound), (rows, n, float(np.max(np.abs(got - want) - bound)))


def test_bad_arguments_are_refused(rbpf):
    dy, W = _inputs(4, 3, 5)
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.pack_whiten_probe(dy, W, dy_layout=1)
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.pack_whiten_probe(dy[:, :2], W[:2, :2])
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
