"""tests/valcheck.assert_values: the comparison every GPU value test goes through must itself reject what
a wrong kernel would produce -- NaN for a finite value (a `>` test is false for NaN), inf for a finite
value, the wrong signed zero, an error just above the tolerance -- and accept what the rule allows."""
import numpy as np
import pytest

from valcheck import assert_values

SUM, MIN, MAX, COUNT = 0, 1, 2, 3
FLOATS = [np.float32, np.float64]


def _nan(dtype, payload):
    """a quiet NaN with `payload` in its low mantissa bits"""
    if dtype == np.float32:
        return np.array([0x7FC00000 | payload], np.uint32).view(np.float32)[0]
    return np.array([0x7FF8000000000000 | payload], np.uint64).view(np.float64)[0]


def _rejects(got, want, dtype, op, exact=False):
    with pytest.raises(AssertionError):
        assert_values(np.array(got, dtype), np.array(want, dtype), dtype, op, exact)


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("op,exact", [(SUM, False), (SUM, True), (MIN, False), (MAX, False)])
def test_rejects_nan_and_inf_mismatches(dtype, op, exact):
    for got, want in (([1.0, np.nan], [1.0, 2.0]), ([1.0, 2.0], [1.0, np.nan]), ([np.inf, 1.0], [3.0, 1.0]),
                      ([3.0], [np.inf]), ([-np.inf], [np.inf]), ([np.nan], [np.inf]), ([np.inf], [np.nan])):
        _rejects(got, want, dtype, op, exact)
    # a result that is NaN everywhere
    _rejects([np.nan] * 4, [0.5, 1.5, 2.5, 3.5], dtype, op, exact)


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("op,exact", [(SUM, True), (MIN, False), (MAX, False)])
def test_rejects_wrong_signed_zero_when_exact(dtype, op, exact):
    _rejects([0.0], [-0.0], dtype, op, exact)
    _rejects([-0.0], [0.0], dtype, op, exact)
    assert_values(np.array([-0.0, 0.0], dtype), np.array([-0.0, 0.0], dtype), dtype, op, exact)


@pytest.mark.parametrize("dtype", FLOATS)
def test_float_sum_tolerance(dtype):
    want = np.array([1.0, -3.0, 1000.0, 0.0], dtype)
    assert_values((want.astype(np.float64) * (1 + 5e-6)).astype(dtype), want, dtype, SUM)
    assert_values((want.astype(np.float64) * (1 - 5e-6)).astype(dtype), want, dtype, SUM)
    _rejects(want.astype(np.float64) * (1 + 2e-5), want, dtype, SUM)
    _rejects(want.astype(np.float64) * (1 - 2e-5), want, dtype, SUM)
    _rejects([1e-20], [0.0], dtype, SUM)                   # the floor of the tolerance is 1e-30 * 1e-5
    assert_values(np.array([0.0], dtype), np.array([-0.0], dtype), dtype, SUM)   # within tolerance: not exact
    # the same errors are differences under MIN / MAX / exact
    _rejects(want.astype(np.float64) * (1 + 5e-6), want, dtype, MIN)
    _rejects(want.astype(np.float64) * (1 + 5e-6), want, dtype, SUM, exact=True)


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("op,exact", [(SUM, False), (SUM, True), (MIN, False), (MAX, False)])
def test_accepts_nan_payloads_and_equal_specials(dtype, op, exact):
    a, b = _nan(dtype, 1), _nan(dtype, 0x155)
    assert a.tobytes() != b.tobytes() and np.isnan(a) and np.isnan(b)
    got = np.array([a, np.inf, -np.inf, 2.0], dtype)
    want = np.array([b, np.inf, -np.inf, 2.0], dtype)
    assert got.tobytes() != want.tobytes()
    assert_values(got, want, dtype, op, exact)


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("op", [SUM, MIN, MAX, COUNT])
def test_integers_bit_exact(dtype, op):
    lim = np.iinfo(dtype)
    want = np.array([lim.min, lim.max, 0, -1], dtype)
    assert_values(want.copy(), want, dtype, op)
    _rejects([lim.min, lim.max, 0, 0], want, dtype, op)
    _rejects([lim.min + 1, lim.max, 0, -1], want, dtype, op)


def test_count_of_float_values_is_integer_exact():
    want = np.array([3, 1, 7], np.int64)
    assert_values(want.copy(), want, np.float32, COUNT)
    with pytest.raises(AssertionError):
        assert_values(np.array([3, 1, 8], np.int64), want, np.float32, COUNT)


def test_reports_count_and_first_offenders():
    want = np.arange(10, dtype=np.float64)
    got = want.copy()
    got[[2, 7]] = np.nan
    with pytest.raises(AssertionError) as e:
        assert_values(got, want, np.float64, SUM)
    msg = str(e.value)
    assert "2 of 10" in msg and "[2]" in msg and "[7]" in msg and "nan" in msg


def test_rejects_shape_and_dtype_mismatch():
    with pytest.raises(AssertionError):
        assert_values(np.zeros(3), np.zeros(4), np.float64, SUM)
    with pytest.raises(AssertionError):
        assert_values(np.zeros(3, np.float32), np.zeros(3, np.float64), np.float64, SUM)
