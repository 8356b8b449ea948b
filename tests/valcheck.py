"""One comparison of per-vertex values with a reference, shared by the GPU tests (a plain module).

The rule (README, "parity"):
  integer dtypes, COUNT, float MIN / MAX, or exact=True:  bit for bit wherever the reference is not NaN
      (signed zeros included); where the reference is NaN the result is NaN.  The NaN payload is not
      compared: Java specifies only "the result is NaN", and which NaN survives depends on combine order.
  float SUM:  NaN exactly where the reference is NaN; equal where the reference is infinite; finite and
      within 1e-5 relative where it is finite.  Every comparison is written with <= / ==, so a NaN fails.
"""
import numpy as np

FLOAT_RTOL = 1e-5   # north star: float weight sums within 1e-5 relative of the arrival-order fold
OP_SUM = 0
_SHOW = 5


def _uint(a):
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _report(bad, got, want, what):
    idx = np.flatnonzero(bad)
    rows = ", ".join(f"[{i}] got {got[i]!r} want {want[i]!r}" for i in idx[:_SHOW])
    raise AssertionError(f"{len(idx)} of {len(want)} values {what}: {rows}")


def assert_values(got, want, dtype, op, exact=False):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{got.shape} values, the reference has {want.shape}"
    assert got.dtype == want.dtype, f"values are {got.dtype}, the reference is {want.dtype}"
    flt = np.issubdtype(np.dtype(dtype), np.floating) and np.issubdtype(want.dtype, np.floating)
    if not flt:
        bad = _uint(got) != _uint(want)
        if bad.any():
            _report(bad, got, want, "differ (bit-exact required)")
        return
    wn, gn = np.isnan(want), np.isnan(got)
    if exact or op != OP_SUM:
        bad = np.where(wn, ~gn, _uint(got) != _uint(want))
        if bad.any():
            _report(bad, got, want, "differ (bit-exact required, NaN for NaN)")
        return
    g, w = got.astype(np.float64), want.astype(np.float64)
    wi = np.isinf(w)
    with np.errstate(invalid="ignore"):
        near = np.isfinite(g) & (np.abs(g - w) <= FLOAT_RTOL * np.maximum(np.abs(w), 1e-30))
    ok = np.where(wn, gn, np.where(wi, g == w, near))
    if not ok.all():
        _report(~ok, got, want, "outside 1e-5 relative (NaN for NaN, inf for inf)")
