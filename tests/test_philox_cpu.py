"""CPU checks behind the random-draw tests: the from-spec Philox4x32-10 of philox_ref.py on the published Random123
vectors, the host transcription PhiloxRNG.backward_uniforms against it, and the strict left-to-right order of np.cumsum
that test_gpu_resample_edges.py takes as tools/sample.m:30's `cumsum(w)`."""
import numpy as np
import pytest

import philox_ref as P


@pytest.mark.parametrize("counter,key,want", P.KNOWN_ANSWERS)
def test_philox4x32_10_known_answers(counter, key, want):
    assert P.philox4x32_10(counter, key) == want


def test_known_answers_notice_a_wrong_constant_or_key_order():
    """The vectors pin every constant: each single-constant change, and swapped key halves, miss the third vector."""
    counter, key, want = P.KNOWN_ANSWERS[2]
    assert P.philox4x32_10(counter, key[::-1]) != want
    for name in ("M0", "M1", "W0", "W1"):
        old = getattr(P, name)
        try:
            setattr(P, name, old ^ 2)
            assert P.philox4x32_10(counter, key) != want, name
        finally:
            setattr(P, name, old)
    assert P.philox4x32_10(counter, key) == want


def test_unit53_rounds_at_the_top_as_ieee_doubles_do():
    """(a + 0.5) * 2^-53: exact below a = 2^52, rounded to even from there on, so u lies in (0, 1] and 1.0 is reached."""
    assert P._unit53(0, 0) == 2.0 ** -54
    assert P._unit53(0xFFFFFFFF, 0xFFFFFFFF) == 1.0                     # a = 2^53 - 1: a + 0.5 rounds up to 2^53
    assert P._unit53(0xFFFFFFFF, 0xFFFFF000) == 1.0 - 2.0 ** -52        # a = 2^53 - 2: a + 0.5 rounds down to a (even)
    assert P._unit53(0x7FFFFFFF, 0xFFFFF800) == 0.5 - 2.0 ** -54        # a = 2^52 - 1: still exact


@pytest.mark.parametrize("seed", P.SEEDS)
def test_host_backward_uniforms_equal_the_spec(rbpf, seed):
    M, T = 5, 4
    got = rbpf.PhiloxRNG(seed).backward_uniforms(M, T)
    assert got.shape == (T, M) and got.dtype == np.float64
    want = np.array([[P.uniform2(seed, j, t, P.BACKWARD_LANE, 0)[0] for j in range(M)] for t in range(T)])
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 1e-18              # the Box-Muller reference needs the extended format


def test_normals_reference_layout():
    """Pairs on lanes 1, 2, ...; an odd count uses the cosine half of the last pair; r is the pair's radius."""
    z8, r8 = P.normals(7, 3, 2, 1, 8)
    z3, r3 = P.normals(7, 3, 2, 1, 3)
    np.testing.assert_array_equal(z3, z8[:3])
    for j in range(0, 8, 2):
        u0, _ = P.uniform2(7, 3, 2, 1 + j // 2, 1)
        assert abs(float(z8[j] ** 2 + z8[j + 1] ** 2) - (-2.0 * np.log(u0))) < 1e-14
        assert r8[j] == r8[j + 1] and abs(float(r8[j]) ** 2 - (-2.0 * np.log(u0))) < 1e-14


def test_numpy_cumsum_is_strictly_sequential():
    """np.cumsum(w)[j] == ((w0 + w1) + w2) + ... + wj in doubles, on weights spread over many binades (pairwise or
    blocked summation would differ at most indices)."""
    rs = np.random.RandomState(3)
    w = np.exp(-40.0 * rs.random_sample(20000))
    w /= w.sum()
    run, want = 0.0, np.empty_like(w)
    for j, v in enumerate(w.tolist()):
        run += v
        want[j] = run
    np.testing.assert_array_equal(np.cumsum(w), want)
    blocked = np.concatenate([np.cumsum(w[b:b + 1024]) for b in range(0, w.size, 1024)])
    off = np.concatenate(([0.0], np.cumsum(blocked[1023::1024])))[: (w.size + 1023) // 1024]
    blocked += np.repeat(off, 1024)[: w.size]
    assert np.mean(blocked != want) > 0.5                    # the check can tell the two orders apart
