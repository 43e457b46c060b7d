"""CPU self-check of the comparison helper of tests/test_gpu_nonfinite.py: the mistakes it exists to catch make it fail."""
import numpy as np
import pytest

from test_gpu_nonfinite import check_against_oracle


def _want():
    return np.array([1.0, np.nan, np.inf, -np.inf, -0.0, 0.0, 4.9e-324, 2.5, -3.0])


def test_helper_accepts_the_oracle_itself_and_a_result_within_tolerance():
    w = _want()
    check_against_oracle(w.copy(), w, tol=0.0)
    check_against_oracle(w.copy(), w, bitwise=True)
    g = w.copy()
    g[7] = 2.5 * (1 + 1e-13)
    check_against_oracle(g, w, tol=1e-12)
    with pytest.raises(AssertionError, match="relative error"):
        check_against_oracle(g, w, tol=1e-15)
    with pytest.raises(AssertionError, match="bits"):
        check_against_oracle(g, w, bitwise=True)
    c = np.array([1 + 2j, complex(np.nan, np.inf)])
    check_against_oracle(c.copy(), c, tol=0.0)


def test_helper_rejects_a_moved_nan():
    w = _want()
    g = w.copy()
    g[1], g[0] = 1.0, np.nan
    for kw in (dict(tol=1.0), dict(bitwise=True), dict(atol=1e300)):
        with pytest.raises(AssertionError, match="NaN positions"):
            check_against_oracle(g, w, **kw)


def test_helper_rejects_an_inf_of_the_wrong_sign():
    w = _want()
    g = w.copy()
    g[2] = -np.inf
    for kw in (dict(tol=1.0), dict(bitwise=True)):
        with pytest.raises(AssertionError, match="Inf positions"):
            check_against_oracle(g, w, **kw)


def test_helper_rejects_a_lost_sign_of_zero_and_a_flushed_subnormal_in_bitwise_mode():
    w = _want()
    g = w.copy()
    g[4] = 0.0
    assert np.array_equal(g[[0, 4, 5]], w[[0, 4, 5]])           # == cannot see it
    with pytest.raises(AssertionError, match="bits"):
        check_against_oracle(g, w, bitwise=True)
    g = w.copy()
    g[6] = 0.0
    with pytest.raises(AssertionError, match="bits"):
        check_against_oracle(g, w, bitwise=True)
    w32 = np.array([-0.0, 1e-40], np.float32)
    with pytest.raises(AssertionError, match="bits"):
        check_against_oracle(np.array([0.0, 1e-40], np.float32), w32, bitwise=True)
